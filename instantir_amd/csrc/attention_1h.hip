// Flash-style attention for ONE head of dimension D = 128 / 256 / 512 (the mid-block attention of AutoencoderKL: D is the block's
// channel count, 512 for SDXL, 128 for VAEConfig.tiny()), bf16 or fp16 in / fp32 scores, softmax statistics and accumulation /
// 16-bit out, gfx950.
//
// Replaces the three GEMMs around a row softmax that HipVAE._attention runs per image (T x T fp32 scores and T x T 16-bit
// probabilities through memory, a ceiling of 16384 keys): one launch for the whole batch, nothing of size T x T anywhere, any
// Tq >= 1 and Tkv >= 1.  Data contract: Q[b][t][d] and K[b][t][d] token-major with row strides, V consumed transposed
// (Vt[d][b*vbs + t], rows readable on [0, roundup8(Tkv)); what lies at and past Tkv may be anything, NaN bit patterns included),
// O[b][t][d] = softmax(Q K^T * scale) V + o_bias[d].
//
// Per workgroup: NW waves x 16 query rows (NW = 4: 64 rows; NW = 2: 32 rows when the 64-row grid would leave CUs idle), 32-key
// tiles, K and V^T tiles double-buffered in LDS by global_load_lds_dwordx4 (4 x 64 D bytes: 128 KiB at D = 512).
//   S^T = K . Q^T with 16x16x32 MFMA: keys on the accumulator rows, the query on the lane (lane & 15), Q fragments held in
//     registers for the whole kernel (D/32 k-steps x 4 VGPRs).
//   O^T += V^T . P^T with 16x16x32 MFMA: d on the accumulator rows in D/16 blocks, one k-step = the 32 keys of the tile; the
//     packed P registers are the B operand as they stand.
// LDS row (kb, m) of the K image holds key 8*(m >> 2) + 4*kb + (m & 3) of the tile, so accumulator register i of key block kb on
// lane group gq = lane >> 4 is the score of key 8*gq + 4*kb + i: a lane's 8 scores are the 8 CONSECUTIVE keys 8*gq + [0, 8) that
// the lane supplies as k-slots of the second product, and a V^T fragment is one 16-byte read.
// LDS images: one 1 KiB block per MFMA operand fetch, laid out in lane order (byte 16 * lane of the block is that lane's fragment),
// so a glds16 instruction fills exactly one block and every ds_read_b128 reads 1 KiB contiguous: conflict-free with no swizzle.
//   K image  [D/32 k-steps][2 key blocks][lane (gq, m)][16 B]: d = 32*ks + 8*gq + [0, 8) of LDS row (kb, m)
//   V^T image [D/16 d blocks][lane (gq, m)][16 B]:             keys 8*gq + [0, 8) of row d = 16*db + m
//
// Softmax: the running maximum is updated every tile and the accumulators rescaled by exp2(m_old - m_new) whenever any row's
// maximum moved (exact for scores arbitrarily far apart).  The row sum is kept per lane over the lane's own keys and the four
// lane groups are added once at the end in a fixed order; no atomics, bit-identical run to run.
//
// DESIGN 5.8 rule: no cross-lane exchange downstream of a per-lane-guarded load.  Every load here is unconditional from a clamped
// address (query row, key row, V^T column chunk).  Keys at and past Tkv get a score of -inf (P = 0), and the V^T fragments of the
// last tile are ANDed with a per-lane key mask after the LDS read, so a masked key contributes 0 x 0, never 0 x NaN.
#include "common.h"
#include "../../include/instantir_hip.h"
#include <type_traits>

namespace {

constexpr int KT1 = 32;       // keys per tile

struct Geo1 {
    const void* Q; long ldq, qbs;
    const void* K; long ldk, kbs;
    const void* Vt; long ldvt, vbs;
    void* O; long ldo, obs;
    const void* bias;
    int Tq, Tkv, qtiles;
    float c;                  // softmax scale * log2(e)
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <typename E, int D, int NW>
__global__ __launch_bounds__(64 * NW) void attn_1h_kernel(const Geo1 g) {
    using x8 = typename ET<E>::x8;
    using x4 = typename ET<E>::x4;
    constexpr int KS = D / 32;            // k-steps of S^T = K . Q^T
    constexpr int NDB = D / 16;           // 16-row blocks of O^T = blocks of one tile image
    constexpr int IMG = KT1 * D * 2;      // bytes of one K tile image, and of one V^T tile image
    constexpr int FB = 4;                 // fragment blocks per read batch
    static_assert(D % 32 == 0 && NDB % NW == 0 && NDB % FB == 0, "head_dim must be a multiple of 32 and of 16 * NW");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                      // [2][NDB blocks][1 KiB]
    char* Vs = smem + 2 * IMG;            // [2][NDB blocks][1 KiB]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, gq = lane >> 4;
    const int b = blockIdx.x / g.qtiles;
    const int q0 = (blockIdx.x % g.qtiles) * (16 * NW) + wave * 16;
    const int qq = q0 + n;

    // Q fragments: B operand of S^T = K . Q^T -- lane (n, gq) holds d = 32*ks + 8*gq + [0, 8) of query n (row clamped)
    x8 qf[KS];
    {
        const int q = qq < g.Tq ? qq : g.Tq - 1;
        const E* qp = (const E*)g.Q + (long)b * g.qbs + (long)q * g.ldq + 8 * gq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const x8*)(qp + 32 * ks);
    }

    const E* kbase = (const E*)g.K + (long)b * g.kbs + 8 * gq;
    const E* vbase = (const E*)g.Vt + (long)b * g.vbs + (long)n * g.ldvt;
    const int ntiles = (g.Tkv + KT1 - 1) / KT1;

    // one tile: NDB K blocks and NDB V^T blocks, one glds16 each, spread over the waves.  Key rows past the end repeat the last
    // key (masked by the tile body); a V^T chunk wholly past the end reads the image's column 0 (masked as well).
    auto stage = [&](int t, int buf) {
        {
            const int k0 = t * KT1 + 8 * (n >> 2) + (n & 3);
#pragma unroll
            for (int j = 0; j < NDB / NW; ++j) {
                const int i = wave + j * NW, ks = i >> 1, kb = i & 1;
                int key = k0 + 4 * kb;
                key = key < g.Tkv ? key : g.Tkv - 1;
                glds16(kbase + (long)key * g.ldk + 32 * ks, Ks + buf * IMG + i * 1024);
            }
        }
        {
            int col = t * KT1 + 8 * gq;
            col = col < g.Tkv ? col : 0;
#pragma unroll
            for (int j = 0; j < NDB / NW; ++j) {
                const int i = wave + j * NW;
                glds16(vbase + (long)(16 * i) * g.ldvt + col, Vs + buf * IMG + i * 1024);
            }
        }
    };

    float m = -INFINITY, l = 0.f;
    f32x4 o[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntiles) stage(t + 1, buf ^ 1);
        const char* kt = Ks + buf * IMG + lane * 16;
        const char* vt = Vs + buf * IMG + lane * 16;

        // ---- S^T = K . Q^T: register i of block kb is key 8*gq + 4*kb + i of the tile
        // (fragment reads go FB blocks at a time, the next batch issued before the MFMAs of the current one: with one wave per
        //  SIMD at d = 512 nothing else hides the LDS round trip)
        f32x4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        x8 fr[2][FB];
#pragma unroll
        for (int j = 0; j < FB; ++j) fr[0][j] = *(const x8*)(kt + j * 1024);
#pragma unroll
        for (int bt = 0; bt < NDB / FB; ++bt) {
            if (bt + 1 < NDB / FB) {
#pragma unroll
                for (int j = 0; j < FB; ++j) fr[(bt + 1) & 1][j] = *(const x8*)(kt + ((bt + 1) * FB + j) * 1024);
            }
#pragma unroll
            for (int j = 0; j < FB; ++j) {
                const int i = bt * FB + j;              // block (ks, kb) = (i >> 1, i & 1)
                s[i & 1] = ET<E>::mfma16(fr[bt & 1][j], qf[i >> 1], s[i & 1]);
            }
        }
        const bool tail = (t + 1) * KT1 > g.Tkv;          // (wave-uniform) keys past the end in this tile
        const int key0 = t * KT1 + 8 * gq;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[kb][i] *= g.c;
                if (tail && key0 + 4 * kb + i >= g.Tkv) s[kb][i] = -INFINITY;
            }
        // ---- online softmax (base 2); key 32*t is inside the segment for every tile, so the row maximum is finite
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        if (__any(m_new > m)) {
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);       // (first tile: exp2(-inf) = 0 on zeros)
            l *= alpha;
#pragma unroll
            for (int i = 0; i < NDB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[i][r] *= alpha;
            m = m_new;
        }
        x8 pf;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = __builtin_amdgcn_exp2f(s[kb][i] - m);
                l += p;
                pf[4 * kb + i] = (E)p;
            }

        // ---- O^T += V^T . P^T: lane (n, gq) supplies keys 8*gq + [0, 8); accumulator register r of block db is d = 16*db + 4*gq + r
        //      (the key mask is all ones except in a tile that reaches past the end)
        u32x4 vm = {~0u, ~0u, ~0u, ~0u};
        if (tail) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                vm[j] = (key0 + 2 * j < g.Tkv ? 0x0000FFFFu : 0u) | (key0 + 2 * j + 1 < g.Tkv ? 0xFFFF0000u : 0u);
        }
        auto pv = [&](auto masked) {
            u32x4 fv[2][FB];
#pragma unroll
            for (int j = 0; j < FB; ++j) fv[0][j] = *(const u32x4*)(vt + j * 1024);
#pragma unroll
            for (int bt = 0; bt < NDB / FB; ++bt) {
                if (bt + 1 < NDB / FB) {
#pragma unroll
                    for (int j = 0; j < FB; ++j) fv[(bt + 1) & 1][j] = *(const u32x4*)(vt + ((bt + 1) * FB + j) * 1024);
                }
#pragma unroll
                for (int j = 0; j < FB; ++j) {
                    const int db = bt * FB + j;
                    const u32x4 raw = decltype(masked)::value ? fv[bt & 1][j] & vm : fv[bt & 1][j];
                    o[db] = ET<E>::mfma16(__builtin_bit_cast(x8, raw), pf, o[db]);
                }
            }
        };
        if (!tail) pv(std::false_type{});
        else pv(std::true_type{});
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
    }

    // ---- normalise, add the bias, store: lane (n, gq) holds d = 16*db + 4*gq + [0, 4) of query n
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (qq < g.Tq) {
        E* op = (E*)g.O + (long)b * g.obs + (long)qq * g.ldo + 4 * gq;
        const E* bp = (const E*)g.bias + 4 * gq;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (g.bias) {
                const x4 bb = *(const x4*)(bp + 16 * db);
#pragma unroll
                for (int r = 0; r < 4; ++r) bv[r] = (float)bb[r];
            }
            x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (E)(o[db][r] * inv + bv[r]);
            *(x4*)(op + 16 * db) = v;
        }
    }
}

template <typename E, int D, int NW>
int launch_1h(const Geo1& g0, int batch, hipStream_t stream) {
    Geo1 g = g0;
    g.qtiles = (g.Tq + 16 * NW - 1) / (16 * NW);
    const size_t lds = 4 * (size_t)KT1 * D * 2;
    static unsigned long long lds_set = 0;
    if (!iir_ensure_dynamic_lds((const void*)attn_1h_kernel<E, D, NW>, lds, lds_set)) return IIR_ELAUNCH;
    iir_launch(attn_1h_kernel<E, D, NW>, dim3((unsigned)(batch * g.qtiles)), dim3(64 * NW), lds, stream, g);
    return iir_launch_status();
}

template <typename E, int D>
int launch_1h_rows(const Geo1& g, int batch, hipStream_t stream) {
    // 64 query rows per workgroup, 32 while that leaves the 64-row grid below one workgroup per CU (256 CUs)
    const long wg64 = (long)batch * ((g.Tq + 63) / 64);
    return wg64 >= 256 ? launch_1h<E, D, 4>(g, batch, stream) : launch_1h<E, D, 2>(g, batch, stream);
}

template <typename E>
int launch_1h_dim(const Geo1& g, int batch, int head_dim, hipStream_t stream) {
    switch (head_dim) {
        case 128: return launch_1h_rows<E, 128>(g, batch, stream);
        case 256: return launch_1h_rows<E, 256>(g, batch, stream);
        case 512: return launch_1h_rows<E, 512>(g, batch, stream);
        default: return IIR_EINVAL;
    }
}

}  // namespace

extern "C" int iir_attention_1h(const iir_attn_desc* a, int32_t head_dim, int32_t dtype, const void* o_bias, void* stream) {
    if (!a || !a->Q || !a->O) return IIR_EINVAL;
    if (a->heads != 1 || a->nseg != 1 || a->causal || a->o_fp8 || a->q_prescaled) return IIR_EINVAL;
    if (head_dim != 128 && head_dim != 256 && head_dim != 512) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    const iir_attn_kv* s = &a->kv[0];
    if (!s->K || !s->Vt) return IIR_EINVAL;
    if (a->Tq < 1 || s->Tkv < 1 || a->batch < 1) return IIR_EINVAL;
    if (a->ldq % 8 || a->q_batch_stride % 8 || a->ldo % 8 || a->o_batch_stride % 8) return IIR_EINVAL;
    if (s->ldk % 8 || s->k_batch_stride % 8 || s->ldvt % 8 || s->vt_batch_stride % 8) return IIR_EINVAL;
    if (a->ldq < head_dim || a->ldo < head_dim || s->ldk < head_dim || s->ldvt < ((s->Tkv + 7) & ~7)) return IIR_EINVAL;
    if ((uintptr_t)a->Q % 16 || (uintptr_t)s->K % 16 || (uintptr_t)s->Vt % 16 || (uintptr_t)a->O % 8 || (uintptr_t)o_bias % 8) return IIR_EINVAL;
    if (!(a->scale > 0.f)) return IIR_EINVAL;
    if ((long)a->batch * ((a->Tq + 31) / 32) > 0x7fffffffL) return IIR_EINVAL;
    (void)hipGetLastError();
    Geo1 g{};
    g.Q = a->Q; g.ldq = a->ldq; g.qbs = a->q_batch_stride;
    g.K = s->K; g.ldk = s->ldk; g.kbs = s->k_batch_stride;
    g.Vt = s->Vt; g.ldvt = s->ldvt; g.vbs = s->vt_batch_stride;
    g.O = a->O; g.ldo = a->ldo; g.obs = a->o_batch_stride;
    g.bias = o_bias;
    g.Tq = a->Tq; g.Tkv = s->Tkv;
    g.c = a->scale * 1.4426950408889634f;
    return dtype == IIR_DT_BF16 ? launch_1h_dim<bf16>(g, a->batch, head_dim, (hipStream_t)stream)
                                : launch_1h_dim<f16>(g, a->batch, head_dim, (hipStream_t)stream);
}
