/* libinstantir_hip.so -- C ABI of the MI355X (gfx950) kernels behind the InstantIR denoising path.
 *
 * The reference (rebots-online/InstantIR) is pure Python on PyTorch ops; it has no FFI of its own
 * (SURVEY.md section 8b).  Each entry point below therefore replaces a *call site* of a PyTorch op in
 * the reference and cites it.  Conventions: plain C symbols, raw device pointers, explicit
 * dims/strides (element counts, fp16 unless noted), `stream` is a hipStream_t passed as void*,
 * caller owns every buffer, return 0 on success, IIR_EINVAL (-1) for rejected arguments,
 * IIR_ELAUNCH (-2) when the launch failed.  No global state besides one-time kernel attributes;
 * thread-safe per stream; nothing here allocates, synchronises or copies, so every entry point may
 * be captured into a hipGraph.
 *
 * Activation layout is NHWC / (rows, tokens, channels): a (R, C, H, W) reference tensor is the
 * (R, H, W, C) buffer here, which is also the (R, H*W, C) token matrix (reference permutes at
 * module/min_sdxl.py:581-583,590-594 -- free here).
 */
#ifndef INSTANTIR_HIP_H
#define INSTANTIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IIR_ABI_VERSION 3

/* epilogue selectors */
#define IIR_EPI_PLAIN 0 /* C = act(acc + bias + rowbias) + res                                    */
#define IIR_EPI_GEGLU 1 /* C[:, j] = (acc_v + b_v) * gelu_erf(acc_g + b_g); W rows pair-permuted  */
#define IIR_EPI_SFT 2   /* C[:, j] = res[:, j] * (acc_gamma + b + 1) + (acc_beta + b)             */
#define IIR_EPI_XATTN 3 /* C = cross_attention(q = acc + bias, xattn_kv[0], xattn_kv[1]): see iir_gemm_desc.xattn_kv */
#define IIR_ACT_NONE 0
#define IIR_ACT_SILU 1
#define IIR_ACT_GELU 2 /* erf form */
#define IIR_ACT_QUICKGELU 3 /* x * sigmoid(1.702 x), CLIP-L text encoder */

/* Pair permutation expected by GEGLU / SFT epilogues: for an op with `n_out` outputs whose
 * "value" rows are V[0..n_out) and partner rows are G[0..n_out), the weight (and bias) handed to
 * the kernel has 2*n_out rows where rows [16*b, 16*b+8) = V[8*b, 8*b+8) and
 * rows [16*b+8, 16*b+16) = G[8*b, 8*b+8).  (Host helper: instantir_amd.packing.pair_rows.) */

#define IIR_DT_F16 0
#define IIR_DT_BF16 1

typedef struct iir_attn_kv {
    const void* K; int64_t ldk, k_batch_stride;     /* K[b][t][h*64+d]                               */
    const void* Vt; int64_t ldvt, vt_batch_stride;  /* Vt[h*64+d][b*vt_batch_stride + t]; rows finite */
    int32_t Tkv;                                    /*   and readable on [0, roundup8(Tkv))           */
} iir_attn_kv;

typedef struct iir_gemm_desc {
    const void* A; int64_t lda;    /* [M][K] activations, row stride lda                           */
    const void* W;                 /* [N][K] weights (torch nn.Linear layout), K contiguous        */
    void* C; int64_t ldc;          /* [M][N] (or [M][N/2] for paired epilogues)                    */
    int32_t M, N, K;               /* K % 64 == 0, N % 4 == 0                                      */
    const void* bias;              /* [N] or NULL                                                  */
    const void* rowbias; int64_t ldrb; int32_t rows_per_rb; /* + rowbias[m / rows_per_rb][n]       */
    const void* res; int64_t ldr;  /* residual / SFT `h` input, or NULL                            */
    int32_t epi, act;
    float out_scale;               /* 0 means 1                                                    */
    int32_t tile;                  /* 0 auto; base shape 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 128x160, 5 = 64x160, 6 = 256x128 (8 waves), */
                                   /*   ring depth and loader waves chosen by the library; or one build by id: base + 10 x stages           */
                                   /*   (21-26, 31, 34-36), loader waves 54 (128x160) / 55, 65, 75 (64x160, 3 / 4 / 2 stages), 90 = 256x320 */
                                   /*   (paired epilogues), 91 / 92 = the 8-wave kernel at BN 320 / 256.  Any other value: IIR_EINVAL.      */
    const void* prefetch;          /* optional: range the workgroups touch (at most 1024 128-byte lines each) */
    int64_t prefetch_bytes;        /*   so it is in the Infinity Cache for a LATER launch (next layers' weights) */
    void* Ct; int64_t ldct;        /* optional (PLAIN epilogue, no residual on those columns): output columns n >= tr_from */
    int32_t tr_from;               /*   are stored TRANSPOSED, Ct[(n - tr_from) * ldct + m] -- the V third of a fused       */
                                   /*   q|k|v projection lands as the V^T image iir_attention_d64_f16 consumes              */
    int32_t dtype;                 /* IIR_DT_F16 (0) or IIR_DT_BF16 (1): element type of A, W, C, bias, rowbias, res.  The  */
                                   /*   bf16 build serves the VAE, which the reference runs in fp32 because the SDXL VAE   */
                                   /*   overflows fp16 (pipelines/sdxl_instantir.py:984-1001,1668-1674)                     */
    int32_t c_f32;                 /* != 0: C is float [M][N] (ldc in floats, plain epilogue, out_scale only): the VAE     */
                                   /*   mid-block attention scores stay fp32 through their softmax                          */
    const void* wscale;            /* != NULL: W holds fp8-E4M3 (OCP) BYTES [N][K] and wscale[n] (fp32, 16-byte aligned) is */
                                   /*   the scale of row n: C = epi((A8 . W8^T) * wscale[n] ...), A converted to fp8 in the */
                                   /*   kernel (BASELINE configs[4]: "fp8 MFMA weights" for the LCM single-step path)       */
    /* LayerNorm without a LayerNorm launch (nn.LayerNorm -> nn.Linear pairs of BasicTransformerBlock, module/min_sdxl.py:541-562):  */
    void* ln_stats_out;            /* producer side, optional: the launch that WRITES the residual stream also leaves, per row and   */
                                   /*   per column tile, (mean, M2) of the fp16 values it stored: float2 [iir_gemm_ln_parts()][M]    */
    const void* ln_stats_in;       /* consumer side, optional: A holds the RAW (un-normalised) rows; W must be W . diag(gamma),      */
    int32_t ln_parts, ln_part_cols;/*   bias must carry W . beta; the kernel merges the `ln_parts` partials of each row (each over   */
    float ln_eps;                  /*   `ln_part_cols` columns; parts x cols == K) to (mean, rstd) and forms                         */
    const void* ln_colsum;         /*   C = epi(rstd * (A . W^T) - rstd * mean * ln_colsum[n] + bias ...), ln_colsum[n] = sum_k W[n][k] (fp32) */
    /* GroupNorm statistics from the launch that produces the GroupNorm's input (nn.Conv2d / proj_out -> nn.GroupNorm pairs,          */
    /* module/min_sdxl.py:242-283,565-595): no separate statistics pass over the tensor                                               */
    void* gn_stats_out;            /* optional (PLAIN epilogue, whole tiles, M % 64 == 0): float2 [M / 64][N] = (mean, M2) of the 64   */
                                   /*   stored values of every channel per 64-row slab; consumed by iir_groupnorm_from_partials       */
    /* IIR_EPI_XATTN: the Linear is `attn2.to_q` of TA_IPAttnProcessor2_0 (module/ip_adapter/attention_processor.py:1140) with the     */
    /* softmax scale x log2(e) folded into W / bias by the caller; every workgroup finishes a 64-row x 2-head tile of q and runs the    */
    /* two SDPA calls + add of :1165,:1185,:1192 on it, so C receives `hidden_states + ip_hidden_states` (before to_out) and q never     */
    /* goes to memory.  Needs: fp16, N % 128 == 0 (head dimension 64), M % 64 == 0, xattn_tq % 64 == 0, 1 <= Tkv[0] <= 80,             */
    /* 1 <= Tkv[1] <= 64, ldk / ldvt / batch strides % 8 == 0, no res / rowbias / act / Ct / c_f32 / wscale / *_stats_out.                */
    /* out_scale multiplies the finished fp16 output (C = fp16(fp16(O) * out_scale)), never q.                                          */
    const iir_attn_kv* xattn_kv;   /* [2]: text K / V^T, IP-token K / V^T (layouts as for iir_attention_d64_f16)                       */
    int32_t xattn_tq;              /* query rows per image (row m belongs to image m / xattn_tq)                                      */
    /* BASELINE configs[4], both operands in fp8: with `wscale` set and a_fp8 != 0, A holds fp8-E4M3 (OCP) BYTES [M][K] too (lda in    */
    /* bytes, % 16; K % 128 == 0): C = epi((A8 . W8^T) * wscale[n] * a_scale ...).  Half the 128-byte lines per FLOP of the fp16 form. */
    int32_t a_fp8;
    float a_scale;                 /* 0 means 1                                                                                       */
    int32_t c_fp8;                 /* != 0: C is a BYTE matrix of fp8-E4M3 (ldc in bytes, % 8; whole tiles; PLAIN / GEGLU epilogues, */
                                   /*   no *_stats_out / Ct / c_f32): the value is rounded to fp16 first, then to fp8 (scale 1)     */
} iir_gemm_desc;

/* Replaces nn.Linear / F.linear call sites: attention projections
 * module/ip_adapter/attention_processor.py:370,377-378,402,1140,1148-1149,1173-1174,1195; GEGLU
 * feed-forward module/min_sdxl.py:502-528; proj_in/out :572,575; time_emb_proj :266; embeddings
 * :226-240; AdaLayerNorm linear attention_processor.py:23; Resampler resampler.py:48-49,66-68,95-97. */
int iir_gemm_f16(const iir_gemm_desc* d, void* stream);
/* partials per row a tile = 0, plain-epilogue launch of (M, N, K) writes to `ln_stats_out`; 0 = that launch cannot (ragged tiles) */
int iir_gemm_ln_parts(int32_t M, int32_t N, int32_t K);
/* the tile `tile = 0` resolves to for an (M, N, K) problem (paired != 0 for GEGLU / SFT epilogues) */
int iir_gemm_pick_tile(int32_t M, int32_t N, int32_t K, int32_t paired);
/* The tile / kernel iir_gemm_f16(d) resolves to, without launching (91: the 8-wave 256x320 kernel of csrc/gemm8.hip, used for the
 * GEGLU projections of module/min_sdxl.py:502-528 when its tiles fill the chip); -1 for an invalid descriptor. */
int iir_gemm_resolve_tile(const iir_gemm_desc* d);
/* 1 when the tile = 0, plain-epilogue fp16 launch of (M, N, K) can leave GroupNorm partials in `gn_stats_out` */
int iir_gemm_gn_supported(int32_t M, int32_t N, int32_t K, int32_t is_conv);
/* 1 when the tile = 0 all-fp8 launch (a_fp8) of (M, N, K) can store its result as fp8 bytes (c_fp8): whole tiles */
int iir_gemm_fp8_out_supported(int32_t M, int32_t N, int32_t K, int32_t paired);
/* output-tile width BN of tile id `tile` (1..6) */
int iir_gemm_tile_bn(int32_t tile);

typedef struct iir_conv_desc {
    const void* X; int64_t ldx;    /* NHWC input (R, H, W, Cin), pixel stride ldx >= Cin           */
    int32_t R, H, Wd, Cin;         /* image count, height, width; Cin % 64 == 0 (host pads latents) */
    const void* Wt;                /* [Cout][k][k][Cin] weights                                    */
    void* Y; int64_t ldy;          /* NHWC output, pixel stride ldy                                */
    int32_t Cout, ksize, stride, upsample;   /* ksize 1|3, stride 1|2, nearest-2x folded if upsample */
    const void* bias;
    const void* rowbias; int64_t ldrb; int32_t rows_per_rb;
    const void* res; int64_t ldr;
    int32_t epi, act;
    float out_scale;
    int32_t tile;
    const void* zero_page;         /* >= 128 zero bytes: source of the padding pixels              */
    int64_t x_img_stride;          /* elements between input images; 0 = H*Wd*ldx (dense)          */
    int32_t y_img_rows;            /* rows between images in Y; 0 = Ho*Wo (dense)                  */
    int32_t res_img_rows;          /* rows between images in res; 0 = Ho*Wo                        */
    int32_t pad_mode;              /* 0: symmetric ksize/2; 1: pad 0 top/left, 1 bottom/right (VAE  */
                                   /*    Downsample2D(padding=0) + F.pad(0,1,0,1), vae.py:110)      */
    const void* prefetch;          /* as in iir_gemm_desc                                          */
    int64_t prefetch_bytes;
    int32_t dtype;                 /* IIR_DT_F16 / IIR_DT_BF16, as in iir_gemm_desc                */
    void* gn_stats_out;            /* as in iir_gemm_desc: float2 [R * Ho * Wo / 64][Cout] (rows of one image must fill whole 64-row slabs) */
} iir_conv_desc;

/* Replaces nn.Conv2d call sites: ResnetBlock2D module/min_sdxl.py:256-259,274 (+ the temb add :267 as
 * `rowbias`, the residual add :279 as `res`), Downsample2D :601-606, Upsample2D :612-618 (with
 * F.interpolate nearest folded in), conv_in/conv_out :827,912, SFT module/aggregator.py:62-67,76-86. */
int iir_conv2d_nhwc_f16(const iir_conv_desc* c, void* stream);

typedef struct iir_attn_desc {
    const void* Q; int64_t ldq, q_batch_stride;     /* Q[b][t][h*64+d]                               */
    void* O; int64_t ldo, o_batch_stride;           /* O[b][t][h*64+d]                               */
    int32_t batch, heads, Tq, nseg;                 /* nseg 1 or 2                                   */
    float scale;                                    /* 1/sqrt(64) for SDPA                           */
    iir_attn_kv kv[2];
    int32_t causal;                                 /* != 0: key j is visible to query i only if j <= i */
    int32_t q_prescaled;                            /* != 0: Q already holds q * scale * log2(e) (the caller folded the factor
                                                     *   into the projection weights); the kernel then uses Q as it stands   */
    int32_t o_fp8;                                  /* != 0: O is a BYTE matrix of fp8-E4M3 (ldo, o_batch_stride in bytes): the
                                                     *   A operand of an all-fp8 `to_out` GEMM (iir_gemm_desc.a_fp8)         */
} iir_attn_desc;

/* Replaces F.scaled_dot_product_attention at module/ip_adapter/attention_processor.py:394 (nseg=1)
 * and the two SDPA calls + add at :1165,:1185,:1192 (nseg=2: text KV, IP KV), head_dim 64. */
int iir_attention_d64_f16(const iir_attn_desc* a, void* stream);
/* The same launch with identity attention on batch rows [ident_from, batch): O[b] = V[b] there (perturbed-attention
 * guidance, PAGIdentitySelfAttnProcessor: the attention map of the perturbed rows is the identity, so the value projection
 * passes through).  V is read from kv[0].Vt, the transposed operand the plain launch reads.  Rows below ident_from are
 * bit-identical to iir_attention_d64_f16.  Needs 1 <= ident_from < batch, nseg == 1, kv[0].Tkv == Tq, not causal, no o_fp8. */
int iir_attention_d64_ident_f16(const iir_attn_desc* a, int32_t ident_from, void* stream);

/* F.scaled_dot_product_attention at head_dim 80 / 104 (CLIP ViT-H/14, bigG/14 vision towers:
 * module/ip_adapter/utils.py:106-118); layouts as iir_attention_d64_f16 with 64 -> head_dim.
 * head_dim 64 is routed to iir_attention_d64_f16. */
int iir_attention_f16(const iir_attn_desc* a, int32_t head_dim, void* stream);

/* Single-head attention of AutoencoderKL's mid block: `Attention(heads=1)` of module/unet/unet_2d_ZeroSFT_blocks.py:776-790,
 * whose SDPA is module/ip_adapter/attention_processor.py:394, at head_dim = the block's channel count (128, 256 or 512).
 * One flash-style launch for the whole batch, nothing of size Tq x Tkv in memory, any Tq >= 1 and Tkv >= 1.
 * dtype: IIR_DT_F16 / IIR_DT_BF16, the element type of Q, K, Vt, O and o_bias (fp32 scores, softmax and accumulation).
 * Layouts as iir_attention_d64_f16 with heads = 1 and 64 -> head_dim; Vt rows must be readable on [0, roundup8(Tkv)) but
 * need not be finite at and past Tkv.  O = softmax(Q K^T * scale) V + o_bias (o_bias: [head_dim] or NULL; rows of the
 * softmax sum to 1, so this is the V projection's bias added after the product).
 * IIR_EINVAL for heads != 1, nseg != 1, causal, o_fp8, q_prescaled, another head_dim or dtype, a null Q / K / Vt / O, a row or
 * batch stride that is not a multiple of 8 elements or a row stride below the row, Tq / Tkv / batch < 1, scale <= 0, and
 * Q / K / Vt not 16-byte (O, o_bias: 8-byte) aligned. */
int iir_attention_1h(const iir_attn_desc* a, int32_t head_dim, int32_t dtype, const void* o_bias, void* stream);

/* nn.GroupNorm (+ fused nn.SiLU) on NHWC: module/min_sdxl.py:245,252,257,269-271,568,841.
 * workspace: iir_groupnorm_workspace_bytes(R, groups) bytes of fp32 partial sums. */
int iir_groupnorm_nhwc_f16(const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t R, int32_t HW, int32_t C,
                           int32_t groups, const void* gamma, const void* beta, float eps, int32_t silu,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* nn.GroupNorm (+ SiLU) whose statistics pass already happened in the producing launch (`gn_stats_out` of iir_gemm_f16 /
 * iir_conv2d_nhwc_f16: float2 [R * HW / 64][ldp] (mean, M2) per 64-row slab and channel): merges the slabs and channels of
 * every (image, group), then normalises X into Y.  HW % 64 == 0.  Same call sites as iir_groupnorm_nhwc_f16. */
int iir_groupnorm_from_partials(const void* partials, int64_t ldp, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t R,
                                int32_t HW, int32_t C, int32_t groups, const void* gamma, const void* beta, float eps, int32_t silu,
                                void* workspace, int64_t workspace_bytes, int32_t dtype, void* stream);
/* the same for fp16 or bf16 tensors (X, Y, gamma, beta of type `dtype`): the VAE's GroupNorms (eps 1e-6,
 * module/diffusers_vae/vae.py via unet_2d_ZeroSFT_blocks.py:2804-2874) run on bf16 activations */
int iir_groupnorm_nhwc(const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t R, int32_t HW, int32_t C,
                       int32_t groups, const void* gamma, const void* beta, float eps, int32_t silu,
                       void* workspace, int64_t workspace_bytes, int32_t dtype, void* stream);
int64_t iir_groupnorm_workspace_bytes(int32_t R, int32_t groups);

/* nn.LayerNorm (module/min_sdxl.py:534-538; resampler.py:15,43-44,98) and AdaLayerNorm's
 * LN(x)*(1+scale)+shift (attention_processor.py:24-25).  gamma/beta/shift/scale may be NULL.
 * transposed == 2 stores y as fp8-E4M3 BYTES (Y a byte matrix, ldy in bytes: the A operand of an all-fp8 GEMM, iir_gemm_desc.a_fp8);
 * transposed == 1 stores y^T (used to emit the IP-adapter V^T image directly):
 *   Y[c][ (row / tr_rows) * tr_bstride + row % tr_rows ], row stride ldy. */
int iir_layernorm_f16(const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t rows, int32_t C, const void* gamma,
                      const void* beta, float eps, const void* shift, const void* scale, int64_t ldmod,
                      int32_t rows_per_mod, int32_t transposed, int32_t tr_rows, int64_t tr_bstride, void* stream);

/* Every adaLN of one UNet forward in one launch.  The IP-adapter tokens are step invariant, so the raw to_k_ip /
 * to_v_ip projections are hoisted; what is left per step and per TA-IP block is AdaLayerNorm(raw, temb)
 * (module/ip_adapter/attention_processor.py:14-26 as called at :1173-1176): LN without affine, then * (1 + scale) + shift.
 * jobs_dev: DEVICE array of njobs records; all jobs share rows, eps, ldmod (row stride of the shift / scale matrix),
 * rows_per_mod, tr_rows and tr_bstride (meaning as in iir_layernorm_f16); max_C = largest C in the table. */
typedef struct iir_adaln_job {
    const void* X; void* Y; const void* shift; const void* scale;
    int64_t ldx, ldy;
    int32_t C, transposed;
} iir_adaln_job;
int iir_adaln_batch_f16(const iir_adaln_job* jobs_dev, int32_t njobs, int32_t rows, int32_t max_C, float eps, int64_t ldmod,
                        int32_t rows_per_mod, int32_t tr_rows, int64_t tr_bstride, void* stream);

/* In-place row softmax (fp32 math) of an fp16 matrix, cols <= 16384: the score matrix of the VAE mid-block
 * attention (1 head of dim 512, T = (H/8)*(W/8) tokens; torch.softmax inside F.scaled_dot_product_attention,
 * module/ip_adapter/attention_processor.py:394 as used by module/unet/unet_2d_ZeroSFT_blocks.py:776-790). */
int iir_softmax_rows_f16(void* X, int64_t ld, int32_t rows, int32_t cols, void* stream);
/* softmax over the columns of fp32 scores S[rows][cols] (cols % 4 == 0, <= 16384) written as fp16 / bf16 probabilities P:
 * the VAE mid-block attention (Attention(heads=1), unet_2d_ZeroSFT_blocks.py:776-790) keeps its scores in fp32 through the
 * softmax like the reference's upcast VAE (pipelines/sdxl_instantir.py:984-1001) */
int iir_softmax_rows_f32(const float* S, int64_t lds, void* P, int64_t ldp, int32_t rows, int32_t cols, int32_t dtype, void* stream);

/* Timesteps: module/min_sdxl.py:205-224.  out[r][col_off + v*dim + ...] = [cos | sin](vals[r][v] * w_k). */
int iir_sinusoid_f16(const float* vals, int32_t n_vals, int32_t rows, int32_t dim, void* out, int64_t ldo,
                     int32_t col_off, void* stream);
int iir_silu_f16(const void* x, void* y, int64_t n, void* stream);

/* dst[m][dst_off + c] = src[m][c] + add[m][c] * add_scale[m / rows_per_scale]: torch.cat of skips
 * (module/min_sdxl.py:712) with the aggregator residual scaling/add folded in
 * (pipelines/sdxl_instantir.py:1602-1603). add / add_scale may be NULL. */
int iir_copy_add_f16(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t dst_off, int64_t M, int32_t C,
                     const void* add, int64_t lda, const float* add_scale, int32_t rows_per_scale, void* stream);

/* FreeU (module/min_sdxl.py:22-77 `fourier_filter` with threshold 1 and `apply_freeu`, applied to each resnet's
 * (hidden, skip) pair before the torch.cat of CrossAttnUpBlock2D / UpBlock2D, module/unet/unet_2d_ZeroSFT_blocks.py:2600-2627,
 * 2748-2775; switched on by `enable_freeu`, unet_2d_ZeroSFT.py:919-949).  Two launches per concat, as the two
 * iir_copy_add_f16 calls they replace.  `rows` = R * H * W NHWC rows of R images; add / add_scale as iir_copy_add_f16 with
 * rows_per_scale = H * W (add_scale may be NULL = 1).
 * iir_freeu_stats_f16: the 7 fp32 sums per (image, channel) of t = skip + add * add_scale that the filter needs (sum t, and
 * sum t cos / sum t sin of the phases of DFT frequencies (1,0), (0,1), (1,1)), per HW slab: partials float
 * [R][IIR_FREEU_SLABS][7][C], iir_freeu_partials_bytes(rows, H, W, C) bytes.
 * iir_freeu_concat_f16 (reads those partials in a fixed order):
 *   cat[m][cat_off + c]      = (x + mid_add * add_scale)[m][c] * (c < cx / 2 ? b : 1),   c < cx
 *   cat[m][cat_off + cx + c] = fourier_filter(skip + add * add_scale, threshold 1, scale s)[m][c], c < cs
 * all in fp32, one fp16 rounding per output; s = 1, b = 1 gives exactly the two iir_copy_add_f16 results. */
#define IIR_FREEU_SLABS 16
int64_t iir_freeu_partials_bytes(int64_t rows, int32_t H, int32_t W, int32_t C);
int iir_freeu_stats_f16(const void* skip, int64_t lds, const void* add, int64_t lda, const float* add_scale, int64_t rows,
                        int32_t H, int32_t W, int32_t C, float* partials, int64_t partials_bytes, void* stream);
int iir_freeu_concat_f16(const void* x, int64_t ldx, int32_t cx, const void* mid_add, int64_t ldm, const void* skip, int64_t lds,
                         int32_t cs, const void* add, int64_t lda, const float* add_scale, int64_t rows, int32_t H, int32_t W,
                         float b, float s, const float* partials, int64_t partials_bytes, void* cat, int64_t ldc,
                         int64_t cat_off, void* stream);

/* Smoothed-energy guidance (SEG, Hong 2024): the 2-D Gaussian blur of the queries of the perturbed batch rows of a self-attention,
 * in place in the q | k buffer of the fused projection, between that GEMM and the (plain) attention launch.
 * `q`: the first perturbed row, 16-byte aligned; `images` images of H * W consecutive rows (the token grid, x fastest) follow;
 * row stride `ldq` elements (ldq % 8 == 0, ldq >= C); columns [0, C) are filtered (C % 8 == 0), each channel on its own:
 *   q'[y][x][c] = sum_j wy[j] * (sum_i wx[i] * q[ry(y + j - ky/2)][rx(x + i - kx/2)][c])
 * rx / ry reflect without repeating the edge (-i -> i, n-1+i -> n-1-i).  wy (ky taps) / wx (kx taps): fp32 device memory, read
 * at launch; ky, kx odd with k / 2 <= extent - 1 (k = 1, weight 1: that axis is left alone).  fp16 in, both passes and the
 * intermediate in fp32, taps summed in index order, one fp16 rounding at the store.  `mean` != 0 (the blur's sigma -> inf
 * limit): q'[.][.][c] = mean over the image's H * W tokens, by a pairwise fp32 tree; wy / wx / ky / kx are not read.
 * Columns [C, ldq), rows outside the `images` images and every other byte keep their bits; no atomics: equal inputs give
 * equal bits.  H, W <= IIR_SEG_MAX_EXTENT.  IIR_EINVAL, before any HIP call, for a NULL or misaligned q, NULL taps, a
 * non-positive extent, C % 8, ldq < C or ldq % 8, an even k, k / 2 > extent - 1 or an extent beyond the limit. */
#define IIR_SEG_MAX_EXTENT 128
int iir_seg_blur_q_f16(void* q, int64_t ldq, int32_t images, int32_t H, int32_t W, int32_t C, const float* wy, int32_t ky,
                       const float* wx, int32_t kx, int32_t mean, void* stream);

/* fp32 NCHW latents <-> fp16 NHWC rows (pipelines/sdxl_instantir.py:1503 cat([latents]*2) = rep 2). */
int iir_pack_latent(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep, float scale,
                    void* stream);
int iir_unpack_latent(const void* in, int64_t ldi, int32_t R, int32_t C, int32_t HW, float* out, void* stream);
/* the same with the 16-bit side as fp16 or bf16 (`dtype`): image / latent hand-over of the bf16 VAE */
int iir_pack_latent_t(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep, float scale,
                      int32_t dtype, void* stream);
int iir_unpack_latent_t(const void* in, int64_t ldi, int32_t R, int32_t C, int32_t HW, float* out, int32_t dtype, void* stream);
/* iir_pack_latent_t with the scale read from device memory (`scale` = device fp32[1]): the sigma schedulers' UNet input
 * c_in * x (scale_model_input, pipelines/sdxl_instantir.py:1503-1504) changes every step, and a host float would be baked
 * into a captured graph.  Same expression as iir_pack_latent_t: equal scales give equal bits. */
int iir_pack_latent_dscale(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep, const float* scale,
                           int32_t dtype, void* stream);

/* CFG + main scheduler step (pipelines/sdxl_instantir.py:1619-1633): one descriptor, one launch.  `groups` states which
 * optional groups the caller means (IIR_STEP_* bits); a set bit with a NULL pointer of its group, a non-NULL pointer of a group
 * whose bit is clear, and a bit outside the four are IIR_EINVAL, so a forgotten pointer never runs another formula silently.
 * noise, x0_out, eps_out and eps_factor are plain optional planes (NULL = absent).
 *
 * The step.  coef = device fp32[8] {guidance, sb, sa, k_x0, k_x, k_eps, k_noise, k_h}, read at launch time:
 *   eps  = cfg ? u + g*(c - u) : c        (u = rows [0, B), c = rows [B, 2B) of eps_nhwc, fp16 NHWC rows of width lde >= C)
 *   x0   = (x - sb*eps)/sa                prev = k_x0*x0 + k_x*x + k_eps*eps + k_noise*noise
 * with sb = sqrt(1-abar_t), sa = sqrt(abar_t) for DDPM (k_eps = 0) and DDIM (k_x = 0).  x, noise, prev, x0_out, eps_out: fp32 NCHW
 * (B, C, H, W), HW = H*W.  eps_out receives the guided eps.
 *
 * eps_factor / iir_cfg_rescale_factor.  rescale_noise_cfg, pipelines/sdxl_instantir.py:181-192 (used at :1623-1626 when
 * guidance_rescale > 0): per image factor[b] = phi * std(eps_text) / std(eps_cfg) + (1 - phi) over (C,H,W); iir_sched_step
 * multiplies the guided eps of image b by eps_factor[b] (NULL = 1; it needs cfg).  coef[0] = guidance scale, as for the step.
 * iir_cfg_rescale_factor reads eps_nhwc, lde, B, C, HW, coef and, under IIR_STEP_PAG, pag_scale -- nothing else of the
 * descriptor, so the descriptor of the step that follows serves both calls.
 *
 * IIR_STEP_PAG (pag_scale).  Perturbed-attention guidance (PAG, Ahn et al. 2024).  The UNet output holds one more group of B
 * rows, the perturbed prediction p: rows [2B, 3B) with cfg, [B, 2B) without.  The guided eps is u + g*(c - u) + s*(c - p) (cfg)
 * or c + s*(c - p), s = *pag_scale (device fp32[1], the step's s_t), formed before the rescale factor is applied
 * (iir_cfg_rescale_factor: the same sum inside eps_cfg).  s == 0 skips the term: the outputs are then bit-identical to the
 * launches without the bit.
 *
 * IIR_STEP_HIST (hist).  One history term, for the Euler / Euler-ancestral / DPM++ 2M schedulers, each in its own sample space:
 * prev = k_x0*x0 + k_x*x + k_eps*eps + k_h*m_prev + k_noise*noise with x0 = (x - sb*eps)/sa
 * (Euler: sb = sigma_i, sa = 1; DPM++: sb = sigma_i/sqrt(sigma_i^2+1), sa = 1/sqrt(sigma_i^2+1)).
 * `hist` = fp32 NCHW (B, C, H, W), updated in place: each element reads m_prev, then stores this step's x0, so one captured
 * launch serves every step.  It is never loaded when k_h == 0 (a solver's first step: the plane may hold garbage).
 * `hist` must not alias x, prev or x0_out, and does not combine with eps_out.  Without the bit coef[7] is ignored.
 *
 * IIR_STEP_KEEP (keep_map, keep_src, keep_noise, keep_coef).  Region-selective restoration (a per-pixel restore map; no
 * reference counterpart -- it extends the CFG + scheduler step of pipelines/sdxl_instantir.py:1619-1633, and "kept" means the
 * trajectory of the LQ latent that :1388-1403 noises to the first timestep):
 *   keep_map   fp32 (B, HW): the map at latent resolution, values in [0, 1] (1 = denoised freely in every step)
 *   keep_src   fp32 NCHW (B, C, H, W): the LQ latent;  keep_noise: fp32 NCHW, the noise that seeded the start of the loop
 *   keep_coef  device fp32[4] {thr, a, b, 0}, read at launch time so that one captured launch serves every step
 * After the update produced prev:  prev[b,c,p] = keep[b,c,p] if keep_map[b,p] <= thr else prev[b,c,p], with
 * keep = a * keep_src + b * keep_noise -- the expression of iir_axpby_f32, bit for bit; a term whose coefficient is 0 is
 * skipped, so {thr, 1, 0} returns the bits of keep_src whatever keep_noise holds.  The caller passes, for step i of N,
 * thr = (N - 1 - i) / N and (a, b) = the add_noise pair of the timetable entry that follows the step ((1, 0) after the last).
 * It is a SELECT on an fp32 compare, never an arithmetic blend: a free element has the bits of the launch without a map, a
 * kept element those of add_noise, and NaN / Inf in a kept pixel's eps never reach prev.  x0_out, hist and eps_out are
 * written exactly as without a map (a multistep solver's history stays the model's own x0).  keep_src and keep_noise may
 * not alias prev.
 *
 * IIR_STEP_APG (apg_avg, apg_sa, apg_par).  The guided eps is the projected form described at iir_apg_project below, with A and
 * {s, alpha} as iir_apg_project left them and eta = apg_par[0]; it needs cfg.  The uncond rows are not read.  The PAG term
 * + s_t*(c - p), eps_factor, the scheduler update, the history term, the noise, x0_out and the restore-map select are as without
 * APG.  With eta = 1, r = 0, beta_t = 0 the eps equals u + w*(c - u) algebraically, not bitwise.  apg_avg may not alias prev,
 * x0_out, eps_out or hist.
 *
 * IIR_EINVAL, before any HIP call: a NULL d, eps_nhwc, coef, x or prev; B, C or HW <= 0; lde < C; eps_factor without cfg; hist
 * equal to x, prev or x0_out; eps_out together with hist; a group bit and its pointers disagreeing, or an unknown bit; keep_src
 * or keep_noise equal to prev; under IIR_STEP_APG cfg == 0 or apg_avg equal to prev, x0_out, eps_out or hist.
 * iir_cfg_rescale_factor: a NULL d, factor, eps_nhwc or coef; B, C or HW <= 0; lde < C; C*HW < 2; IIR_STEP_PAG with a NULL
 * pag_scale. */
#define IIR_STEP_PAG  1u   /* pag_scale: one more group of B perturbed rows in eps_nhwc */
#define IIR_STEP_HIST 2u   /* hist: the k_h * m_prev term; the plane is rewritten with x0 */
#define IIR_STEP_KEEP 4u   /* keep_map, keep_src, keep_noise, keep_coef: restore-map select */
#define IIR_STEP_APG  8u   /* apg_avg, apg_sa, apg_par: projected guidance replaces the CFG sum */

typedef struct iir_sched_desc {
    const void* eps_nhwc; int64_t lde;
    int32_t B, C, HW, cfg;
    const float* coef;
    uint32_t groups;
    const float *x, *noise;  float *prev, *x0_out, *eps_out;  const float* eps_factor;
    const float* pag_scale;  float* hist;
    const float *keep_map, *keep_src, *keep_noise, *keep_coef;
    const float *apg_avg, *apg_sa, *apg_par;
} iir_sched_desc;

int iir_sched_step(const iir_sched_desc* d, void* stream);
int iir_cfg_rescale_factor(const iir_sched_desc* d, float guidance_rescale, float* factor, void* stream);
/* Adaptive projected guidance (APG; Sadat et al., "Eliminating Oversaturation and Artifacts of High Guidance Scales in
 * Diffusion Models"; no reference counterpart -- it replaces the CFG sum of pipelines/sdxl_instantir.py:1619-1621).  Applied to
 * denoised predictions.  Per image b, sums over (C, H, W); u / c = the uncond / cond rows of the UNet output, x the unscaled fp32
 * latent, w = coef[0], sb = coef[1], sa = coef[2] (the vector iir_sched_step reads, either scheduler form):
 *   x0_c = (x - sb*c)/sa            x0_u = (x - sb*u)/sa
 *   D    = x0_c - x0_u
 *   A    = D + beta_t * A_prev      (skipped, and the plane not loaded, when beta_t == 0)
 *   n    = ||A||_2                  s = r > 0 ? min(1, r / n) : 1
 *   alpha= <A, x0_c> / <x0_c, x0_c>                  (0 when x0_c is all zero)
 *   U    = s * (A - (1 - eta) * alpha * x0_c)        (orthogonal part + eta * parallel part, after the clamp)
 *   x0_g = x0_c + (w - 1) * U
 *   eps  = (x - sa*x0_g)/sb         (replaces  u + w*(c - u)  in the step; sb != 0, as at every step of the schedulers here)
 * apg_par = device fp32[4] {eta, r, beta_t, 0}, read at launch time so that one captured launch serves every step;
 * apg_avg = fp32 NCHW (B, C, H, W): A_prev on entry of iir_apg_project, A on exit (each element read, then overwritten, by
 * the thread that owns it); apg_sa = device fp32[2B] {s, alpha} per image.
 * iir_apg_project forms A and {s, alpha}: fp32 element math, fp64 accumulation.  An image is divided among a fixed number of
 * workgroups, each leaving its three partial sums in `workspace` (device, 8-byte aligned, at least
 * iir_apg_project_workspace_bytes(B) bytes, contents undefined afterwards); a second small launch adds an image's partials in
 * index order.  Every order is fixed and there are no atomics: equal inputs give equal bits.  It reads columns [0, C) of rows
 * [0, 2B) of eps_nhwc only.  apg_avg may not be x, apg_sa or the workspace.
 * IIR_EINVAL (before any HIP call): a NULL pointer, B, C or HW <= 0, B > 65535, lde < C, a workspace too small or unaligned. */
int64_t iir_apg_project_workspace_bytes(int32_t B);
int iir_apg_project(const void* eps_nhwc, int64_t lde, int32_t B, int32_t C, int32_t HW, const float* coef, const float* x,
                    const float* apg_par, float* apg_avg, float* apg_sa, void* workspace, int64_t workspace_bytes, void* stream);
/* The restore map at latent resolution: out (B, H / factor, W / factor) = the maximum of map_px (B, H, W) over each
 * factor x factor block (a latent pixel is free if any pixel under it asked for freedom).  fp32; H and W multiples of
 * factor, H, W <= 32768; `out` must not be `map_px`.  IIR_EINVAL for any other geometry, before any launch. */
int iir_map_pool_max_f32(const float* map_px, int32_t B, int32_t H, int32_t W, int32_t factor, float* out, void* stream);
/* Pixel composite of a restored image with its input under a restore map.  decoded, original, out: fp32 planar
 * (B, C, H, W); map_px fp32 (B, H, W).  P = [map_px > 0]; cnt(y, x) = sum of P over the (2r+1) x (2r+1) window with
 * coordinates clamped to the image (replicate edge); w = cnt / (2r+1)^2;
 *   out = decoded where cnt == (2r+1)^2, original where cnt == 0, else w * decoded + (1 - w) * original   (fp32, no FMA)
 * so a pixel whose window lies wholly in the kept region is the input pixel bit for bit.  r = 0 is a hard paste.  Two
 * launches on integer counts: rows into `ws` (iir_region_composite_workspace_bytes(B, H, W) bytes; -1 for a geometry outside
 * the limits), columns fused with the composite.  `out` may equal `decoded`, nothing else.  H, W <= 32768, B * C <= 32767,
 * 0 <= r <= IIR_REGION_MAX_FEATHER; IIR_EINVAL otherwise, before any launch.  No atomics: equal inputs give equal bits. */
#define IIR_REGION_MAX_FEATHER 512
int64_t iir_region_composite_workspace_bytes(int32_t B, int32_t H, int32_t W);
int iir_region_composite_f32(const float* decoded, const float* original, const float* map_px, int32_t B, int32_t C, int32_t H,
                             int32_t W, int32_t r, void* ws, int64_t ws_bytes, float* out, void* stream);
/* LQ fidelity guidance (an addition with no reference call site; lineage and contract in DESIGN.md section 7 "LQ fidelity"):
 * after a scheduler step, pull the step's predicted clean latent toward the LQ latent.  All planes fp32 planar
 * (planes = B * C, H, W), wc = device fp32[2] {w, c}, read at launch:
 *   d = lq - x0_in;  delta = w * LP(d);  x0_out = x0_in + delta;  prev = prev + c * delta;  hist = x0_out (when given)
 * (no FMA contraction in these).  LP is a separable Gaussian of `radius` r, taps[2r + 1] (device fp32, normalised, read at
 * launch), x then y; along each axis the taps that fall outside the image are dropped and the sum is divided by the sum of
 * the taps that stayed:  LPx(d)[y][x] = (sum_j taps[j] * d[y][x + j - r]) / (sum_j taps[j]) over 0 <= x + j - r < W, both sums
 * in index order, the first with fmaf; so LP(const) = const at the borders too.  radius 0: LP is the identity, taps is not
 * read and no filter arithmetic runs.  A workgroup owns an IIR_LQ_FIDELITY_TILE^2 output tile of one plane and stages the tile
 * plus its halo in LDS; neighbours read x0_in through their halos, so x0_out must not be x0_in.  prev and hist are read /
 * written by the thread that owns the pixel.  Every global load is unconditional from a clamped address; no atomics: equal
 * inputs give equal bits.
 * IIR_EINVAL, before any HIP call: a NULL x0_in, lq, wc, prev or x0_out; radius < 0 or > IIR_LQ_FIDELITY_MAX_RADIUS; NULL taps
 * with radius > 0; planes, H or W <= 0 (planes <= 65535, H, W <= 32768); x0_out == x0_in, or any output plane (prev, x0_out,
 * hist) equal to an input plane or to another output plane. */
#define IIR_LQ_FIDELITY_MAX_RADIUS 24
#define IIR_LQ_FIDELITY_TILE 32
int iir_lq_fidelity_f32(const float* x0_in, const float* lq, const float* taps, int32_t radius, const float* wc, int32_t planes,
                        int32_t H, int32_t W, float* prev, float* x0_out, float* hist, void* stream);
/* Batched copy of disjoint byte ranges in one launch: `jobs` = device int64[njobs][3] {src address, dst address, n16}, each
 * job copying n16 x 16 bytes (addresses 16-byte aligned); max_units = the largest n16.  PAG uses it to give the perturbed
 * rows of every Aggregator residual the cond rows' values. */
int iir_copy_segments(const void* jobs, int32_t njobs, int64_t max_units, void* stream);

/* LCMSingleStepScheduler.step, schedulers/lcm_single_step_scheduler.py:455-484.
 * coef = device fp32[4] {sqrt(1-abar_t), sqrt(abar_t), c_out, c_skip}. */
int iir_lcm_step(const void* eps_nhwc, int64_t lde, int32_t B, int32_t rep, int32_t C, int32_t HW, const float* coef,
                 const float* x, void* out_nhwc, int64_t ldo, float* out_nchw, void* stream);

/* Scheduler `.step()` on fp32 NCHW tensors (same linear form as iir_sched_step, no CFG), and
 * a*x + b*y for add_noise (schedulers/lcm_single_step_scheduler.py:492-513; pipelines/sdxl_instantir.py:931-939). */
int iir_sched_step_f32(const float* eps, const float* x, const float* noise, const float* coef, int64_t n, float* prev,
                       float* x0_out, void* stream);
int iir_axpby_f32(const float* x, const float* y, const float* coef, int64_t n, float* out, void* stream);
/* iir_sched_step_f32 with the history term of IIR_STEP_HIST (coef[7] = k_h, `hist` fp32[n] read iff k_h != 0,
 * then overwritten with x0): the sigma schedulers' `.step()`.  `hist` must not alias eps, x, prev or x0_out. */
int iir_sched_step_hist_f32(const float* eps, const float* x, const float* noise, const float* coef, float* hist, int64_t n,
                            float* prev, float* x0_out, void* stream);

/* Weight prefetch: touches every 128-byte line of [p, p+bytes) with `blocks` workgroups so the range
 * sits in the 256 MiB Infinity Cache when the GEMM/conv that streams it starts (the reference has no
 * counterpart: PyTorch streams each layer's weights cold from HBM). */
int iir_prefetch(const void* p, int64_t bytes, int32_t blocks, void* stream);

/* Seam blending of the tiled VAE decode, in place on tile `b` (fp32 NCHW tiles, `planes` = batch*channels):
 * blend_v / blend_h of module/diffusers_vae/autoencoder_kl.py:311-321. */
int iir_blend_tiles_f32(const float* a, float* b, int32_t planes, int32_t Ha, int32_t Wa, int32_t Hb, int32_t Wb,
                        int32_t extent, int32_t vertical, void* stream);

/* LQ-guided colour correction of the decoded image (no reference counterpart: the definitions are the ones StableSR's
 * `wavelet_color_fix` / `adain_color_fix` made standard; contract in DESIGN.md section 7 "Colour fix").  content, style, out:
 * fp32 planar (B, C, H, W) in [0, 1], any H, W >= 1 (<= 32768), B * C <= 32767; `out` may equal `content`.
 *   wavelet: blur_r(x) = replicate-pad by r, depthwise 3x3 [[1,2,1],[2,4,2],[1,2,1]] / 16 at dilation r;
 *            decompose(x): for r in 1, 2, 4, 8, 16: low = blur_r(x), high += x - low, x = low;
 *            out = clamp(decompose(content).high + decompose(style).low, 0, 1), computed as
 *            clamp(content + blur_16(blur_8(blur_4(blur_2(blur_1(style - content)))))), rows then columns (2 launches).
 *   adain:   per (image, channel) over H*W: mean, std = sqrt(unbiased var + 1e-5);
 *            out = clamp((content - mean_c) / std_c * std_s + mean_s, 0, 1); H*W >= 2.  A statistics launch leaves
 *            (n, mean, M2) per slab, float [2][B*C][IIR_COLORFIX_SLABS][3]; the apply launch merges them in slab order.
 * `ws`: iir_colorfix_workspace_bytes(B, C, H, W) bytes (one fp32 plane set for wavelet, the slab table for adain, whichever
 * is larger; -1 for a geometry outside the limits).  No atomics: equal inputs give equal bits. */
#define IIR_COLORFIX_SLABS 64
int64_t iir_colorfix_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int iir_colorfix_wavelet_f32(const float* content, const float* style, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                             void* ws, int64_t ws_bytes, void* stream);
int iir_colorfix_adain_f32(const float* content, const float* style, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                           void* ws, int64_t ws_bytes, void* stream);

/* One axis of a separable, antialiased resize with PIL's filter definitions: the device form of `Image.resize` at
 * infer.py:31-66 (resize_img, Image.BILINEAR to the working size), infer.py:224-225 (back to the requested output size) and
 * the image processors of SURVEY Appendix A (bicubic shortest-edge resize, centre crop, normalise); contract in DESIGN.md
 * section 7 "Resampling".  A resize is the axis-0 (horizontal) launch followed by the axis-1 (vertical) launch, PIL's order.
 *   src: fp32 planar (N, C, H, W), or with src_u8 uint8 interleaved (N, H, W, C), values kept in 0..255 units.
 *   dst: fp32 planar (N, C, h, w): exactly the output window, dense.
 *   The launch resamples `axis` (0: x, 1: y) from its source size to out_size; the other axis keeps its size.  The tables are
 *   PIL's precompute_coeffs layout on the device: bounds int32[out_size][2] {first tap, tap count}, weights
 *   fp32[out_size][ksize], zero padded.  out[o] = sum_k weights[o][k] * src[first(o) + k] over k < count(o), in index order with
 *   fmaf from 0.  First tap and count are clamped into the source axis, so no table makes the kernel read outside src.
 *   Window (y0, x0, h, w), in the coordinates of this launch's full output (rows: out_size or H, columns: out_size or W): only
 *   those samples are computed and stored.  Then, in this order:
 *     quantize: v = min(max(floor(v + 0.5), 0), 255)   (PIL's 8-bit pass: round half up, clip)
 *     clamp:    v = min(max(v, lo), hi)
 *     scale / bias (device fp32[C], either may be NULL): v = v * scale[c], then v = v + bias[c]   (two roundings)
 * No atomics, no LDS: equal inputs give equal bits, and a windowed launch gives the bits of that window of the full launch.
 * IIR_EINVAL, before any HIP call: a NULL desc, src, dst, bounds or weights; N, C, H, W, out_size or ksize <= 0; H, W or
 * out_size > IIR_RESAMPLE_MAX_SIDE; N * C > 65535; axis not 0 or 1; a window that is empty or not inside the output;
 * h * w or out_size * ksize beyond a 31-bit grid; clamp with lo > hi or NaN; dst overlapping src. */
#define IIR_RESAMPLE_MAX_SIDE 32768
typedef struct {
    const void* src; int32_t src_u8;
    float* dst;
    int32_t N, C, H, W;
    int32_t axis, out_size;
    const int32_t* bounds; const float* weights; int32_t ksize;
    int32_t y0, x0, h, w;
    int32_t quantize, clamp; float lo, hi;
    const float* scale; const float* bias;
} IirResampleDesc;
int iir_resample_pass(const IirResampleDesc* desc, void* stream);

/* Full-reference image quality, per image: MSE (for PSNR) and SSIM with the definitions restoration papers use (basicsr's
 * calculate_psnr / calculate_ssim); no reference counterpart, contract in DESIGN.md section 7 "Image metrics".
 *   a, b: two images of one shape, N images of C in {1, 3} channels, each independently fp32 planar (N, C, H, W) on a [0, 1]
 *     scale or, with a_u8 / b_u8, uint8 interleaved (N, H, W, C).  All arithmetic is in 0..255 units: an fp32 source is
 *     multiplied by 255 (fp32), and with a_quantize / b_quantize then taken to min(max(floor(v + 0.5), 0), 255) in fp32, the
 *     8-bit image that would be saved; without the flag nothing is rounded.  The flags are ignored for a uint8 source.
 *   crop_border = c >= 0: c pixels are dropped on every side of both images first; H' = H - 2c, W' = W - 2c.
 *   y_channel (C = 3): both images become the one channel Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255, not rounded.
 *   MSE  = mean of (a - b)^2 over every remaining channel and pixel (PSNR = 10 log10(255^2 / MSE) is the caller's, in fp64).
 *   SSIM = per channel, the mean over the (H' - 10) x (W' - 10) positions at which the 11 x 11 window lies inside the image of
 *     (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, with the
 *     windowed moments mu = E[.], s = E[.^2] - mu^2, s12 = E[ab] - mu1 mu2 under the window g g^T, g_j = exp(-(j - 5)^2 / 4.5)
 *     normalised to sum 1; then the mean over channels.
 *   what: IIR_METRIC_PSNR (the MSE), IIR_METRIC_SSIM, or both; the MSE alone runs no filter.
 *   out: double[N][2] = {MSE, SSIM}; an entry that `what` leaves out is written as NaN.
 *   ws: iir_image_metrics_workspace_bytes(desc) bytes, 8-byte aligned: two fp64 partial sums per workgroup (-1 for a
 *     descriptor whose geometry this entry refuses; the pointers are not looked at).
 * A workgroup owns an IIR_METRICS_TILE^2 tile of one SSIM map, filters the five moments of its tile (taps in index order,
 * fmaf from 0, along x then y; the moments are taken about 128, which variances and covariances do not see) and sums its map
 * values and the squared differences of its own pixels in a fixed order; a second launch adds the partial sums in fp64.  No
 * atomics: equal inputs give equal bits.  With two 8-bit sources (uint8 or quantised) and no y_channel the sum of squared
 * differences is exact: the MSE carries the rounding of its final division alone.
 * IIR_EINVAL, before any HIP call: a NULL desc, a, b, out or ws; N, C, H or W <= 0; H or W > 32768; C not 1 or 3; y_channel
 * with C = 1; crop_border < 0; `what` 0 or with a bit outside the two; H' or W' <= 0, or < 11 when SSIM is asked for;
 * N * channels > 65535 or a grid beyond 31 bits; ws too small or ws / out not 8-byte aligned. */
#define IIR_METRICS_TILE 32
#define IIR_METRIC_PSNR 1u
#define IIR_METRIC_SSIM 2u
typedef struct {
    const void* a; const void* b;
    int32_t a_u8, b_u8;
    int32_t a_quantize, b_quantize;
    int32_t N, C, H, W;
    int32_t crop_border, y_channel;
    uint32_t what;
    void* ws; int64_t ws_bytes;
    double* out;
} iir_metrics_desc;
int64_t iir_image_metrics_workspace_bytes(const iir_metrics_desc* d);
int iir_image_metrics(const iir_metrics_desc* d, void* stream);

/* Synthetic degradation: the three operations of the Real-ESRGAN second-order chain (utils/degradation_pipeline.py:230-336,
 * which runs them through basicsr's filter2D, random_add_gaussian_noise_pt and DiffJPEG) that resampling does not cover;
 * contract here and in DESIGN.md section 7 "Synthetic degradation".  Images are fp32 planar (N, C, H, W), contiguous, in
 * [0, 1].  All three: every global load is unconditional from a clamped address, only stores are guarded, no atomics, sums in
 * a fixed order, multiply-adds written as fmaf and nothing else fused: equal inputs give equal bits.
 *
 * iir_filter2d_f32: per-image k x k correlation with reflect padding (no edge pixel repeated), the reference's filter2D:
 *   out[n,c,y,x] = sum_i sum_j taps[n,i,j] * in[n,c,refl(y + i - r),refl(x + j - r)],  r = (ksize - 1) / 2,
 *   refl(t) = -t for t < 0, 2 (L - 1) - t for t >= L;  i the outer and j the inner loop, both in index order, fmaf from 0.
 *   taps: device fp32 (N, ksize, ksize), read at launch.  A workgroup owns an IIR_FILTER2D_TILE^2 output tile of one plane and
 *   stages the tile, its halo and the image's taps in LDS.
 *   IIR_EINVAL, before any HIP call: a NULL in, taps or out; N, C, H or W <= 0; H or W > 32768; N * C > 65535; ksize even,
 *   < 1 or > IIR_FILTER2D_MAX_KSIZE; H <= r or W <= r (one reflection must do); out overlapping in (neighbours read it).
 *
 * iir_add_gaussian_noise_f32: out = min(max(in + (sigma[n] / 255) * z, 0), 1), sigma device fp32[N] in 0..255 units (the
 *   caller keeps it in [0, 255]), z a pure function of (seed, noise_stream, n, c, y, x), whatever the launch geometry:
 *     (r0, r1, r2, r3) = Philox4x32-10(counter = (y * W + x, n, gray ? 0 : c, noise_stream), key = (seed low 32, seed high 32))
 *     u1 = ((float)(r0 >> 8) + 0.5f) * 2^-24,  u2 = ((float)(r1 >> 8) + 0.5f) * 2^-24      (fp32, round to nearest even)
 *     z  = sqrtf(-2 logf(u1)) * cospif(2 u2)
 *   The sum (r >> 8) + 0.5 is exact below 2^23 and has 25 significant bits from there on, where it rounds to the even
 *   neighbour; u is therefore in (0, 1], u1 = 1 (one r0 >> 8 in 2^24) gives z = 0, and |z| <= sqrt(50 ln 2) < 5.9.  The fp64
 *   restatement starts from these fp32 u1, u2.  With `gray` the channels of a pixel share z.  sigma[n] / 255, its product
 *   with z and the sum with `in` are three fp32 roundings.  out may be in (pointwise).
 *   IIR_EINVAL, before any HIP call: a NULL in, sigma or out; N, C, H or W <= 0; H * W >= 2^32; more than 2^31 - 1 workgroups
 *   of 256 elements; out overlapping in without being equal to it.
 *
 * iir_jpeg_roundtrip_f32: what a baseline 4:2:0 JPEG encode + decode at quality q = quality[n] (device fp32[N], clamped to
 *   [1, 99] by the kernel) does to an image, without entropy coding (the role of DiffJPEG(differentiable=False)); C must be 3.
 *   In fp32, in this order (every fmaf is one rounding, every other operation rounds on its own):
 *     R, G, B = 255 * min(max(v, 0), 1)
 *     Y  = fmaf(0.114, B, fmaf(0.587, G, 0.299 * R))
 *     Cb = fmaf(0.5, B, fmaf(-0.331264, G, -0.168736 * R)) + 128
 *     Cr = fmaf(-0.081312, B, fmaf(-0.418688, G, 0.5 * R)) + 128
 *     the image is extended to a multiple of 16 by edge replication (the clamped address);
 *     chroma sample (i, j) = ((p[2i][2j] + p[2i][2j+1]) + (p[2i+1][2j] + p[2i+1][2j+1])) * 0.25
 *     per 8 x 8 block X (sample - 128), with D[u][k] = a(u) cos((2k + 1) u pi / 16), a(0) = sqrt(1/8), a(u > 0) = 1/2, formed
 *     in fp64 and rounded to fp32, every sum over k = 0..7 in index order with fmaf from 0:
 *       t[y][v] = sum_k D[v][k] X[y][k];   c[u][v] = sum_k D[u][k] t[k][v]                      (u: vertical frequency)
 *       f = (q < 50 ? 5000 / q : 200 - 2 q) / 100;   step = T[u][v] * f;   c' = rintf(c / step) * step   (ties to even)
 *       s[u][x] = sum_k D[k][x] c'[u][k];  X'[y][x] = sum_k D[k][y] s[k][x];   sample' = X' + 128
 *     T: ITU-T T.81 Annex K table K.1 for Y, K.2 for Cb / Cr, neither rounded nor clamped after scaling;
 *     chroma upsampled by replication;  d_b = Cb' - 128, d_r = Cr' - 128
 *     R = fmaf(1.402, d_r, Y');  G = fmaf(-0.714136, d_r, fmaf(-0.344136, d_b, Y'));  B = fmaf(1.772, d_b, Y')
 *     out = min(max(., 0), 255) / 255
 *   One wave per 16 x 16 MCU, four per workgroup; a wave loads nothing but its own MCU and all of it before its first store,
 *   so out may be in.
 *   IIR_EINVAL, before any HIP call: a NULL in, quality or out; C != 3; N, H or W <= 0; N > 65535; H or W > 32768; out
 *   overlapping in without being equal to it. */
#define IIR_FILTER2D_MAX_KSIZE 21
#define IIR_FILTER2D_TILE 32
int iir_filter2d_f32(const float* in, const float* taps, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ksize, float* out,
                     void* stream);
int iir_add_gaussian_noise_f32(const float* in, const float* sigma, int32_t N, int32_t C, int32_t H, int32_t W, uint64_t seed,
                               uint32_t noise_stream, int32_t gray, float* out, void* stream);
int iir_jpeg_roundtrip_f32(const float* in, const float* quality, int32_t N, int32_t C, int32_t H, int32_t W, float* out,
                           void* stream);

/* LPIPS v0.1, net = vgg: the perceptual distance the reference builds as `lpips.LPIPS(net='vgg')` at losses/losses.py:81-95,
 * on the device; contract here and in DESIGN.md section 7 "LPIPS".  The thirteen 3x3 convs of VGG-16 `features` run through
 * iir_conv2d_nhwc_f16 with a bias and IIR_ACT_NONE on an (a, b) pair stacked as one batch; the three entries below are what
 * lies between those convs.  16-bit tensors are fp16 or bf16 by `dtype` (IIR_DT_*), NHWC rows; all arithmetic is fp32 unless
 * stated.  All three: every global load is unconditional from a clamped address and masked in registers, only stores are
 * guarded, 64-bit offsets, no atomics, sums in a fixed order: equal inputs give equal bits.
 *
 * iir_lpips_prep (the scaling layer in front of the first conv, losses/losses.py:81-95): src is one of the sources of
 *   iir_image_metrics, N images of 3 channels, fp32 planar (N, 3, H, W) on a [0, 1] scale or, with src_u8, uint8 interleaved
 *   (N, H, W, 3).  x = u / 255 (one fp32 division) for uint8, the stored fp32 value otherwise, so a uint8 image and its fp32
 *   copy give equal bits; then in fp64  s_c = ((2 x - 1) - affine[c]) / affine[3 + c]  with affine = device fp64[6]
 *   {shift[3], scale[3]} (LPIPS: shift -0.030, -0.088, -0.188; scale 0.458, 0.448, 0.450), rounded to fp32 and then to the
 *   16-bit type.  out: (N * H * W) rows of pixel stride ldo; columns [0, 3) receive s, columns [3, IIR_LPIPS_CPAD) zeros (the K
 *   tile the conv's first layer reads), columns past that keep their bits.  The affine is NOT folded into the first conv: the
 *   conv zero-pads in the scaled space.
 *   IIR_EINVAL, before any HIP call: a NULL src, affine or out; N, H or W <= 0; H or W > 32768; ldo < IIR_LPIPS_CPAD or
 *   ldo % 8; out not 16-byte aligned; another dtype; a grid beyond 31 bits; out overlapping src.
 *
 * iir_relu_f16 (the nn.ReLU after each conv that is neither tapped nor pooled, losses/losses.py:81-95): in place over the
 *   (rows, C) matrix x of row stride ld; a negative value, -0 and -inf included, becomes +0, everything else (NaN too) keeps
 *   its bits; columns [C, ld) are not touched.
 *   IIR_EINVAL, before any HIP call: a NULL or not 16-byte aligned x; rows or C <= 0; C % 8; ld < C or ld % 8; another dtype;
 *   a grid beyond 31 bits.
 *
 * iir_lpips_tap (one tap of losses/losses.py:81-95: nn.ReLU, normalize_tensor, the 1x1 `lin` layer, the spatial average; and
 *   the nn.MaxPool2d(2, 2) the features go on through): x holds the tapped conv's PRE-activation rows (bias added, no ReLU)
 *   of 2 * pairs images of H x W pixels and C channels, pixel stride ldx: images [0, pairs) are the `a` half, image
 *   pairs + i is the `b` partner of image i.  Per pair and pixel p, with a = relu(x_a(p)), b = relu(x_b(p)):
 *     ra = 1 / (sqrt(sum_c a_c^2) + 1e-10), rb likewise;  d(p) = sum_c lin_w[c] * (a_c * ra - b_c * rb)^2
 *     out[pair] = (sum_p d(p)) / (H * W)                     (double[pairs])
 *   so a pixel whose channels are all zero gives 0.  Products into sums are fmaf; a lane sums its 8 channels in index order,
 *   the C / 8 lanes of a pixel add by a butterfly; d(p) of a 2x2 quad are added in fp32 in raster order, quads in fp64 (a
 *   workgroup in a fixed order into ws, then a second launch over ws in index order).
 *   dmap (optional): fp32 (pairs, H, W) receives d(p): LPIPS's spatial=True.
 *   pooled (optional; H, W >= 2): (2 * pairs) images of (H / 2) x (W / 2) pixels (floor: an odd last row or column is scored
 *   and not pooled), pixel stride ldp, stacked as x is: the channel-wise maximum of relu(x) over each 2x2 quad, exact.  It is
 *   formed from the registers the distance was formed from: a tapped activation is read once.
 *   lin_w: device fp32[C].  ws: iir_lpips_tap_workspace_bytes(pairs, H, W, C) bytes, 8-byte aligned (-1 for a geometry this
 *   entry refuses).
 *   IIR_EINVAL, before any HIP call: a NULL x, lin_w, ws or out; pairs, H, W or C <= 0; pairs > 65535; H or W > 32768;
 *   C % 8 or C > IIR_LPIPS_MAX_C; ldx < C or ldx % 8; x not 16-byte aligned; pooled with H or W < 2, ldp < C, ldp % 8 or not
 *   16-byte aligned; ws too small or ws / out not 8-byte aligned; another dtype; pooled or dmap overlapping x. */
#define IIR_LPIPS_CPAD 64
#define IIR_LPIPS_MAX_C 512
int iir_lpips_prep(const void* src, int32_t src_u8, int32_t N, int32_t H, int32_t W, const double* affine, void* out, int64_t ldo,
                   int32_t dtype, void* stream);
int iir_relu_f16(void* x, int64_t ld, int64_t rows, int32_t C, int32_t dtype, void* stream);
int64_t iir_lpips_tap_workspace_bytes(int32_t pairs, int32_t H, int32_t W, int32_t C);
int iir_lpips_tap(const void* x, int64_t ldx, int32_t pairs, int32_t H, int32_t W, int32_t C, const float* lin_w, int32_t dtype,
                  float* dmap, void* pooled, int64_t ldp, void* ws, int64_t ws_bytes, double* out, void* stream);

/* DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity", TPAMI 2020; VGG-16), the device
 * part; no reference counterpart, contract here and in DESIGN.md section 7 "DISTS".  For images a, b as (N, 3, H, W) on a
 * [0, 1] scale:
 *   stage 0 is the raw image x itself, fp32, never rounded to a 16-bit type;
 *   the trunk input is h = (x - mean) / std, mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225): iir_lpips_prep with
 *     shift = 2 mean - 1 and scale = 2 std;
 *   stage 1 is convs 0, 2 of torchvision's VGG-16 `features`, each followed by ReLU (64 channels); stages 2..5 apply L2
 *     pooling to the stage before and then convs (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28), each followed by ReLU
 *     (128, 256, 512, 512 channels); a stage's feature is what its last ReLU leaves: 3 + 64 + 128 + 256 + 512 + 512 = 1475
 *     channels in all;
 *   L2 pooling, per channel:  out(i, j) = sqrt(sum_{di, dj in {-1, 0, 1}} g[di] g[dj] x(2i + di, 2j + dj)^2 + 1e-12),
 *     g = (0.25, 0.5, 0.25) (np.hanning(5)[1:-1], outer product, normalised), zero padding, stride 2, pad 1: output sides
 *     ceil(H / 2), ceil(W / 2);
 *   score: with n = H_k W_k pixels per channel c of stage k, mu_a, mu_b the means, s_a^2 = E[a^2] - mu_a^2 (s_b^2 likewise),
 *     s_ab = E[ab] - mu_a mu_b:  S1 = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1),  S2 = (2 s_ab + c2) / (s_a^2 + s_b^2 + c2),
 *     c1 = c2 = 1e-6;  DISTS = 1 - sum_c (alpha_c S1_c + beta_c S2_c) / (sum alpha + sum beta).  The divisions by n, S1, S2 and
 *     the weighting are the host side's (instantir_amd/dists.py, torch fp64 on the device); the entries below give raw sums.
 * The thirteen convs run through iir_conv2d_nhwc_f16 with a bias and IIR_ACT_NONE on an (a, b) pair stacked as one batch, as
 * for LPIPS.  16-bit tensors are fp16 or bf16 by `dtype` (IIR_DT_*), NHWC rows with a pixel stride.  All entries: every global
 * load is unconditional from a clamped address and masked in registers, only stores are guarded, 64-bit offsets, no atomics,
 * sums in an order that depends on the geometry alone: equal inputs give equal bits.
 *
 * iir_dists_l2pool: x holds a stage's last conv's PRE-activation rows (bias added, no ReLU; as iir_lpips_tap takes them) of
 *   `images` images of H x W pixels and C channels, pixel stride ldx; the ReLU is applied on read.  out: (images, ceil(H / 2),
 *   ceil(W / 2), C) of pixel stride ldo in the same 16-bit type; columns [C, ldo) keep their bits.  Arithmetic is fp32: the
 *   squares of 16-bit values and the power-of-two weights are exact, the nine terms are added in raster order of (di, dj), then
 *   + 1e-12f, sqrtf, one rounding to the 16-bit type.  A tap outside the image is multiplied by 0.  H = W = 1 is legal.
 *   IIR_EINVAL, before any HIP call: a NULL or not 16-byte aligned x or out; images, H, W or C <= 0; H or W > 32768; C % 8 or
 *   C > IIR_LPIPS_MAX_C; ldx or ldo < C or % 8; another dtype; out overlapping x; a grid beyond 31 bits.
 *
 * iir_dists_stats: x is stacked as for iir_lpips_tap: 2 * pairs images of H x W pixels and C channels, pixel stride ldx, images
 *   [0, pairs) the `a` half, image pairs + i the `b` partner of image i; PRE-activation rows, the ReLU on read; columns
 *   [C, ldx) are never read.  out: double[pairs][C][IIR_DISTS_STATS] = {sum a, sum b, sum a^2, sum b^2, sum ab} over the H * W
 *   pixels.  Every product and every sum is fp64 from the first element: a 16-bit value converts exactly and the product of two
 *   is exact in fp64, so the only error is the summation's, at most (n - 1) 2^-53 sum |terms|.  A lane adds the pixels it
 *   strides through in index order, the lanes of a channel group add by a fixed tree in LDS, each workgroup leaves a partial in
 *   ws, and a second launch adds the partials in a fixed order; the share of a workgroup depends on H * W and C alone, so `pairs` = 2 gives
 *   each pair the bits of its own launch.
 *   ws: iir_dists_stats_workspace_bytes(pairs, H, W, C) bytes, 8-byte aligned (-1 for a geometry this entry refuses).
 *   IIR_EINVAL, before any HIP call: a NULL x, ws or out; pairs, H, W or C <= 0; pairs > 65535; H or W > 32768; C % 8 or
 *   C > IIR_LPIPS_MAX_C; ldx < C or ldx % 8; x not 16-byte aligned; ws too small or ws / out not 8-byte aligned; another dtype;
 *   a grid beyond 31 bits.
 *
 * iir_dists_image_stats: the same five sums for stage 0, read from the two image sources of iir_lpips_prep: N images of 3
 *   channels each, both fp32 planar (N, 3, H, W) on a [0, 1] scale or, with src_u8, both uint8 interleaved (N, H, W, 3) with
 *   x = u / 255 as one fp32 division, so a uint8 image and its fp32 copy give equal bits.  An fp32 value converts to fp64
 *   exactly; a product of two is rounded once (fma into the sum).  out: double[N][3][IIR_DISTS_STATS].  The reduction is
 *   iir_dists_stats' (one template).  ws: iir_dists_image_stats_workspace_bytes(N, H, W) bytes, 8-byte aligned.
 *   IIR_EINVAL, before any HIP call: a NULL src_a, src_b, ws or out; N, H or W <= 0; N > 65535; H or W > 32768; an fp32 source
 *   not 4-byte aligned; ws too small or ws / out not 8-byte aligned; a grid beyond 31 bits. */
#define IIR_DISTS_STATS 5
int iir_dists_l2pool(const void* x, int64_t ldx, int32_t images, int32_t H, int32_t W, int32_t C, int32_t dtype, void* out,
                     int64_t ldo, void* stream);
int64_t iir_dists_stats_workspace_bytes(int32_t pairs, int32_t H, int32_t W, int32_t C);
int iir_dists_stats(const void* x, int64_t ldx, int32_t pairs, int32_t H, int32_t W, int32_t C, int32_t dtype, void* ws,
                    int64_t ws_bytes, double* out, void* stream);
int64_t iir_dists_image_stats_workspace_bytes(int32_t N, int32_t H, int32_t W);
int iir_dists_image_stats(const void* src_a, const void* src_b, int32_t src_u8, int32_t N, int32_t H, int32_t W, void* ws,
                          int64_t ws_bytes, double* out, void* stream);

/* NIQE (Mittal et al. 2013, as basicsr's calculate_niqe restates the MATLAB release), the device part: the per-block signed
 * moments of the luma's natural-scene statistics at two scales; no reference counterpart, contract here and in DESIGN.md
 * section 7 "NIQE".  The AGGD fit, the 36 features per block, the Gaussian model and the distance are the host's, in fp64
 * (instantir_amd/niqe.py).
 *   src: one of the sources of iir_image_metrics: N images of C in {1, 3} channels, fp32 planar (N, C, H, W) on a [0, 1] scale
 *     or, with src_u8, uint8 interleaved (N, H, W, C).  crop_border = c >= 0 drops c pixels on every side: H' = H - 2c,
 *     W' = W - 2c.  C = 3 becomes Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255 with R, G, B in 0..255 units (the fp32
 *     operations of iir_image_metrics' y_channel), C = 1 is taken as grey; the grey value is then rounded to
 *     min(max(floor(v + 0.5), 0), 255), and all arithmetic from here is in 0..255 units.
 *   Block grid: nbh = H' / 96, nbw = W' / 96 (floor); the image is the top-left (96 nbh) x (96 nbw) part of the cropped image.
 *     Nothing below sees a pixel outside that part, and no such pixel is read.
 *   Scale 2: the half-size image by MATLAB's imresize(., 0.5) (bicubic, antialiased), which at this factor is the separable
 *     filter [-3, -9, 29, 111, 111, 29, -9, -3] / 256: output o of an axis reads inputs 2o - 3 .. 2o + 4 at symmetric indices
 *     (-1 - i for i < 0, 2n - 1 - i for i >= n), along y first and then along x, taps in index order, fmaf from 0, neither
 *     rounded nor clipped.  Its blocks are 48 x 48 on the same grid.
 *   MSCN, per scale: g_j = exp(-(j - 3)^2 / (2 (7/6)^2)), j = 0..6, normalised to sum 1 in fp64 and rounded to fp32;
 *     mu = G * x, sigma = sqrt(|G * x^2 - mu^2|) with the window applied along x then y (taps in index order, fmaf from 0) and
 *     replicate padding at the edge of the block-grid image; m = (x - mu) / (sigma + 1).  Both moments are taken about 128,
 *     which m does not see.
 *   Per block, five maps: v0 = m and v1..v4 = m * roll(m, s), s = (0, 1), (1, 0), (1, 1), (1, -1) in (row, column), roll the
 *     circular shift within the block (numpy.roll).  Of each map, in this order: the count of v < 0, the count of v > 0, the sum
 *     of v^2 over v < 0, the sum of v^2 over v > 0, the sum of |v|; exact zeros are in neither count.  The 26th value is the
 *     block's sum of sigma.
 *   out: double[N][2][nbh * nbw][IIR_NIQE_STATS], scale 1 first, blocks in raster order; out_bytes its size.
 *   ws: iir_niqe_workspace_bytes(N, C, H, W, crop_border) bytes, 8-byte aligned: the two grey planes (-1 for a geometry this
 *     entry refuses).
 * A thread sums at most 24 values per statistic in fp32, then fp64 in a fixed order; counts are integers.  No atomics: equal
 * inputs give equal bits, and an image's figures do not depend on N.
 * IIR_EINVAL, before any HIP call: a NULL src, ws or out; N, C, H or W <= 0; H or W > 32768; C not 1 or 3; crop_border < 0;
 * H' or W' < IIR_NIQE_BLOCK; N > 65535 or a grid beyond 31 bits; ws or out too small or not 8-byte aligned. */
#define IIR_NIQE_BLOCK 96
#define IIR_NIQE_STATS 26
int64_t iir_niqe_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop_border);
int iir_niqe_stats(const void* src, int32_t src_u8, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop_border, void* ws,
                   int64_t ws_bytes, double* out, int64_t out_bytes, void* stream);

int iir_transpose_f16(const void* in, int64_t ldi, int32_t rows, int32_t cols, void* out, int64_t ldo, int32_t rows_pad,
                      void* stream);
/* Measurement hook (bench.py roofline leg; no reference counterpart): arm a start/stop event pair and the NEXT
 * iir_gemm_f16 / iir_conv2d_nhwc_f16 / iir_attention_d64_f16 launch issued from this thread stamps them with the
 * kernel's own begin / end timestamps on its stream (hipExtLaunchKernelGGL).  After the stream has drained,
 * iir_timing_elapsed_us returns that kernel's duration.  Not usable while the stream is being captured. */
void* iir_timing_event_create(void);
void iir_timing_event_destroy(void* event);
int iir_timing_arm(void* start_event, void* stop_event);
int iir_timing_elapsed_us(void* start_event, void* stop_event, float* us);

int iir_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
