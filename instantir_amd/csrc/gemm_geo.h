// Per-launch constants shared by the GEMM / implicit-GEMM convolution kernels (gemm_conv.hip, gemm8.hip).
#pragma once
#include "common.h"
#include "../../include/instantir_hip.h"
#include <math.h>
#include <type_traits>

namespace iir {

typedef unsigned iir_u32x4 __attribute__((ext_vector_type(4)));
// 16-byte store of an output row chunk.  `wt`: write-through (`buffer_store_dwordx4 ... sc1`).  A GEMM leaves MBs of dirty lines
// in the eight L2s; the kernel's end-of-dispatch release has to write them back before the next (dependent) launch can start --
// time after the last workgroup has finished (MI355X_MICROARCH.md, row publish-large: 8.2 vs 3.0 us for 2 MB per XCD).  The
// consumer is another launch on other XCDs anyway (it reads through the Infinity Cache), so nothing is lost by not keeping the
// lines.
template <typename V>
__device__ __forceinline__ void store16(void* base, long byte_off, const V& v, bool wt) {
    static_assert(sizeof(V) == 16, "16-byte chunk");
    if (wt) {
        __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7FFFFFFF, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(iir_u32x4, v), r, (int)byte_off, 0, 16);
    } else {
        *(V*)((char*)base + byte_off) = v;
    }
}

struct Geo {   // per-launch constants shared by GEMM and CONV paths
    const f16* A; long lda;
    const f16* W;
    f16* C; long ldc;
    int M, N, K;
    const f16* bias;
    const f16* rowbias; long ldrb; int rows_per_rb;
    const f16* res; long ldr;
    int epi, act;
    float out_scale;
    // conv
    int H, Wd, Cin, Ho, Wo, ks, stride, pad, ups;
    const f16* zero;
    long x_img_stride;        // elements between input images
    int y_img_rows, res_img_rows;   // rows between images in C / res (conv mode); 0 = dense
    int tiles_m, tiles_n;
    int xm, rm, rn;           // XCD partition: xm x (8/xm) rectangles of rm x rn tiles
    const char* pf; int pf_lines;   // weight prefetch: 128-byte lines to pull towards the Infinity Cache
    f16* Ct; long ldct; int tr_from, ct_vec;   // columns n >= tr_from are stored transposed: Ct[(n - tr_from) * ldct + m]
    int c_vec, r_vec;               // C / res rows allow 16-byte accesses (ld % 8 == 0, base 16-byte aligned)
    int dtype;                      // IIR_DT_F16 / IIR_DT_BF16: element type of A, W, C, bias, rowbias, res
    int c_f32;                      // C is float (plain epilogue, out_scale only): the VAE's attention scores
    const float* wscale;            // W8 build: W holds fp8-E4M3 bytes [N][K], wscale[n] its per-output-channel scale (fp32)
    // LayerNorm folded into the GEMMs either side of it ("LayerNorm without a LayerNorm launch"):
    float* ln_out;                  // producer: per (column tile, row) partial (mean, M2) of the rows it writes, [N/BN][M] float2
    const float* ln_in;             // consumer: those partials; A holds the RAW rows, W has gamma folded in
    int ln_parts, ln_part_cols;     //   partial count per row and the columns each one covers
    float ln_eps;
    float* gn_out;                  // GroupNorm statistics of the rows this launch writes: [M / 64][N] (mean, M2) per 64-row slab and channel
    int st_wt;                      // write the output through to memory (sc1 stores): nothing is left dirty in the L2s for the end-of-kernel write-back
    const float* ln_colsum;         //   s[n] = sum_k W[n][k] (fp32): y = rstd * (x . w_n) - rstd * mean * s[n] (+ bias, which carries W . beta)
    // IIR_EPI_XATTN (64 x 128 tile): the finished tile is a q projection (two heads x 64 rows, scale x log2 e folded in by the caller);
    // the workgroup runs the text + IP cross-attention of its rows and heads on it and stores the attention output instead
    int xa_on, xa_tq;               // xa_tq: query rows per image (tile rows never straddle an image: xa_tq % 64 == 0)
    const f16* xa_k[2]; long xa_ldk[2], xa_kb[2];       // K[img][t][head * 64 + d]   (segment 0: text, 1: IP tokens)
    const f16* xa_vt[2]; long xa_ldvt[2], xa_vb[2];     // Vt[head * 64 + d][img * vb + t], readable on [0, roundup8(Tkv))
    int xa_tk[2];                   // 1 <= Tkv[0] <= 80, 1 <= Tkv[1] <= 64
    int c_fp8;                      // C is a byte matrix of fp8-E4M3 (ldc in bytes): stored by the fast write-out path only
    int f8; float a_scale;          // all-fp8 build: A and W are E4M3 bytes, K / lda counted in 2-byte units; C = (A8 . W8^T) * wscale[n] * a_scale
};

// ---- what the 4-wave kernel (gemm_conv.hip) and the 8-wave kernel (gemm8.hip) share: the two must agree bit for bit.  Of
// ln_row_stat, epi_act and geglu_pair gemm_conv.hip keeps its own text ("twin of", with the measurements behind each form): as
// calls they grow the scratch of its 256x320 builds or cost its 64x64 builds a wave per SIMD; xhalf_swap
// and form_tag it shares.

// XCD-aware tile order.  Workgroups b, b+8, b+16, ... share an XCD (= one private L2).  The tile grid is cut into 8 rectangles
// (xm x 8/xm), one per XCD, chosen on the host (xcd_partition) to minimise the operand bytes each L2 has to pull over the
// fabric; inside a rectangle tiles walk M fastest so co-resident workgroups share a weight panel.  Placement only affects
// speed, never results.  False: padding workgroup of a ragged rectangle.
__device__ __forceinline__ bool tile_of_block(const Geo& g, int& tm, int& tn) {
    const int bid = (int)blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int rx = xcd % g.xm, ry = xcd / g.xm;
    tm = rx * g.rm + local % g.rm;
    tn = ry * g.rn + local / g.rm;
    return tm < g.tiles_m && tn < g.tiles_n;
}

// The tile grid and its partition: the split with the least bytes each 4 MiB L2 pulls over the fabric.  Inside a rectangle tiles walk M
// fastest, ~64 workgroups are resident per XCD, so its rm x bm rows of A are re-used by successive groups of N-tile columns:
// while they fit `a_keep_bytes` of the L2 they are read once, otherwise once per group.  (PMC: the 128x160 GEMM class read
// 137 MB per launch against 52 MB of operands; kbench 16384x5120x640: 615 -> 679 TFLOP/s.)  The 4-wave kernel's launches count
// 3 MiB; the 8-wave kernel's have never charged a re-read (HUGE_VAL).  Each keeps the model its launches were measured with.
static inline void xcd_partition(Geo& g, int bm, int bn, double a_keep_bytes) {
    g.tiles_m = (g.M + bm - 1) / bm;
    g.tiles_n = (g.N + bn - 1) / bn;
    double best = -1.;
    const double row_bytes = (double)g.K * 2.;
    for (int xm = 1; xm <= 8; xm *= 2) {
        const int xn = 8 / xm;
        const int rm = (g.tiles_m + xm - 1) / xm, rn = (g.tiles_n + xn - 1) / xn;
        const double a_bytes = (double)rm * bm * row_bytes, w_bytes = (double)rn * bn * row_bytes;
        const int cols_per_group = rm >= 64 ? 1 : 64 / rm;
        const double groups = (double)((rn + cols_per_group - 1) / cols_per_group);
        double cost = (a_bytes <= a_keep_bytes ? a_bytes : a_bytes * groups) + w_bytes;
        cost += ((double)rm * rn * 8 - (double)g.tiles_m * g.tiles_n) * 8. * 64 * (bm + bn);     // padding workgroups of ragged rectangles
        if (best < 0. || cost < best) { best = cost; g.xm = xm; g.rm = rm; g.rn = rn; }
    }
}

// LayerNorm statistics (rstd, -rstd * mean) of row m from the producer's per-column-tile partials (ln_in).  Equal-count groups:
// mean = average of the group means, M2 = sum of the group M2 + cols * sum (mean_j - mean)^2; absent groups masked at the merge.
__device__ __forceinline__ float2 ln_row_stat(const Geo& g, int m) {
    constexpr int MAXP = 8;
    float2 lnp_in[MAXP];
#pragma unroll
    for (int j = 0; j < MAXP; ++j) lnp_in[j] = ((const float2*)g.ln_in)[(long)min(j, g.ln_parts - 1) * g.M + m];
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < MAXP; ++j) sm += j < g.ln_parts ? lnp_in[j].x : 0.f;
    const float inv_p = 1.0f / (float)g.ln_parts, mean = sm * inv_p;
    float m2 = 0.f, dev = 0.f;
#pragma unroll
    for (int j = 0; j < MAXP; ++j) {
        const float d = lnp_in[j].x - mean;
        m2 += j < g.ln_parts ? lnp_in[j].y : 0.f;
        dev += j < g.ln_parts ? d * d : 0.f;
    }
    const float var = (m2 + (float)g.ln_part_cols * dev) * inv_p / (float)g.ln_part_cols;
    const float rstd = rsqrtf(var + g.ln_eps);
    return make_float2(rstd, -rstd * mean);
}

// All-fp8 MFMA step: the 16 bytes a lane holds of each operand are 16 K values, fed to two v_mfma_f32_16x16x32_fp8_fp8 (low and
// high 8 bytes: any split of the contraction index is valid as long as both operands use the same one).
template <typename V>
__device__ __forceinline__ f32x4 mfma16_f8x2(V w, V a, f32x4 c) {
    typedef long l2 __attribute__((ext_vector_type(2)));
    const l2 w2 = __builtin_bit_cast(l2, w), a2 = __builtin_bit_cast(l2, a);
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(w2[0], a2[0], c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(w2[1], a2[1], c, 0, 0, 0);
}

// Phase 1 of the epilogue, per accumulator value x (already times the fp8 scales where there are any): the LayerNorm fold
// rs = (rstd, -rstd * mean) -- (1, 0) without ln_in -- about the column sum of W, plus bias; then the activation.
__device__ __forceinline__ float epi_affine(float x, float2 rs, float colsum, float bias) { return fmaf(x, rs.x, fmaf(rs.y, colsum, bias)); }
// The fp32 value as it stands, before the fp16 rounding of the store.  Without it hipcc fuses an fp32 multiply (or fma) and the
// conversion behind it into one v_fma_mixlo_f16 -- a single rounding -- for whichever elements it pleases, build by build,
// while the 4-wave kernel rounds twice (fp32, then fp16): one element in ~2^13 then differs by an fp16 ulp.
__device__ __forceinline__ float rounded_f32(float x) {
    asm("" : "+v"(x));
    return x;
}

// A launch-uniform choice (epilogue form, activation) handed to a generic lambda as a compile-time value: the caller
// tests the flag once and the lambda's body holds no run-time test of it.
template <int V>
using form_tag = std::integral_constant<int, V>;

// (ACT is a compile-time value: the caller decides the activation once per chunk, outside its unrolled quad loops)
template <int ACT>
__device__ __forceinline__ void epi_act(float (&v)[4]) {
    if constexpr (ACT == IIR_ACT_SILU) for (int t = 0; t < 4; ++t) v[t] = silu_f(v[t]);
    else if constexpr (ACT == IIR_ACT_GELU) for (int t = 0; t < 4; ++t) v[t] = gelu_erf_f(v[t]);
    else if constexpr (ACT == IIR_ACT_QUICKGELU) for (int t = 0; t < 4; ++t) v[t] = quick_gelu_f(v[t]);
}

// Cross-half swap (v_permlane32_swap, VALU, no LDS): lanes 0-31 keep `lo` and receive their partner's (lane + 32) `lo` as the
// second value; lanes 32-63 receive their partner's (lane - 32) `hi` as the first value and keep `hi` as the second.
__device__ __forceinline__ void xhalf_swap(float lo, float hi, float& first, float& second) {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
    first = __uint_as_float(s[0]);
    second = __uint_as_float(s[1]);
}

// GEGLU pair step, value * gelu(gate).  A lane (frow, fq) holds 4 consecutive columns `a`; value lanes (fq = 0,1) and their gate
// lanes (fq + 2) sit 32 lanes apart.  The value lane finishes columns 0,1 of the quad (its a[0], a[1] times the gelu of the gate
// lane's a[0], a[1]), its gate lane columns 2,3 (the value lane's a[2], a[3] times the gelu of its own a[2], a[3]): one swap of
// (a[0], a[2]) and one of (a[1], a[3]) hand every lane exactly its (value, gate) pairs.  `geglu_col` is the first of the lane's
// two columns inside the group's 8 output columns.
__device__ __forceinline__ int geglu_col(int fq) { return (fq & 1) * 4 + (fq >= 2 ? 2 : 0); }
template <typename E>
__device__ __forceinline__ auto geglu_pair(const float (&a)[4]) {
    typedef E E2 __attribute__((ext_vector_type(2)));
    float v0, g0, v1, g1;
    xhalf_swap(a[0], a[2], v0, g0);
    xhalf_swap(a[1], a[3], v1, g1);
    return (E2){(E)rounded_f32(v0 * gelu_erf_f(g0)), (E)rounded_f32(v1 * gelu_erf_f(g1))};
}

// Weight prefetch for the launches that follow (see iir_gemm_desc.prefetch): 4-byte LDS-DMA touches of this workgroup's share
// of the `pf_lines` 128-byte lines, clamped into the range; no VGPR destination, the data lands in the wave's 256 B of
// `scratch` behind the ring and is never read.  NT threads, TOUCHES per lane (x 128 B x NT = up to 128-256 KiB per workgroup).
template <int NT, int TOUCHES>
__device__ __forceinline__ void touch_next_weights(const Geo& g, int tid, char* scratch) {
    const int per = (g.pf_lines + (int)gridDim.x - 1) / (int)gridDim.x;
    const long l0 = (long)blockIdx.x * per, last = g.pf_lines - 1;
#pragma unroll
    for (int i = 0; i < TOUCHES; ++i) {
        long l = l0 + min(tid + i * NT, per - 1);
        if (l > last) l = last;
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(g.pf + l * 128), (LDS_AS void*)scratch, 4, 0, 0);
    }
}

// gemm8.hip: 256 x BN tile, 8 waves, two-tile-deep LDS-DMA pipeline (BN = 320 or 256).  Returns IIR_EINVAL when the launch is
// outside what that kernel covers (the caller then takes the 4-wave kernel).
int gemm8_launch(const Geo& g, int bn, hipStream_t stream);
bool gemm8_covers(const Geo& g, int bn);

}  // namespace iir
