// Flash-style attention for head_dim 80 and 104 (OpenCLIP ViT-H/14 and ViT-bigG/14 vision towers), fp16 in / fp32 softmax +
// accumulate / fp16 out, gfx950.
//
// Replaces F.scaled_dot_product_attention inside the CLIP vision tower that `--use_clip_encoder` loads
// (module/ip_adapter/utils.py:106-118).  Same data contract as iir_attention_d64_f16 with 64 -> D: Q[b][t][h*D+d] and
// K[b][t][h*D+d] token-major with given row strides, V consumed transposed (Vt[h*D+d][b*vbs + t], each row readable and finite on
// [0, roundup8(Tkv))), O[b][t][h*D+d], one or two KV segments summed, causal masking and a pre-scaled Q supported.  Kept in a
// file of its own so the d = 64 objects stay as they are; it runs once per image in the encoder, never in the denoising step.
//
// Per workgroup: 4 waves x 32 query rows, 64-key tiles, K and V^T tiles double-buffered in LDS by global_load_lds_dwordx4.
//   S^T = K . Q^T with 32x32x16 MFMA, keys on the accumulator rows and the query on the lane; the MFMA K dimension (d) is padded
//     to DK = roundup16(D): 80 -> 5 k-steps, 104 -> 7 (112).  The pad (d in [104, 112), lane half 1 of the last k-step) is ZERO
//     in both operands, written by the kernel: the Q fragment is loaded from a clamped address and replaced by zeros in
//     registers, and the K fragment comes from a chunk plane of the LDS image that is zeroed once per kernel and never staged.
//     (Columns h*D + [D, DK) of a row belong to the next head or lie past the row, and 0 x Inf = NaN.)
//   O^T += V^T . P^T with 32x32x16 MFMA, d on the accumulator rows in blocks of 32: 80 -> 3 blocks (96 rows), 104 -> 4 (128).
//     V^T image rows [D, DV) are zeroed once per kernel and never staged; only d < D is stored.
// The K rows of a tile are staged in the order both attention kernels use (attn_geo.h, attn_krow_key), so accumulator register
// 8*sp + j of lane half hh is the score of key 32*kb + 16*sp + 8*hh + j: the packed P registers are the B operand as they stand
// and each V^T fragment is one 16-byte read.
//
// LDS layouts (both conflict-free for the ds_read_b128 lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and their +32 twins):
//   K image, CHUNK-MAJOR: [DK/8 planes][64 rows][16 B]; plane c holds halves d = 8c + [0, 8) of every row.  A fragment read is
//     lane qi -> row 32*kb + qi of one plane, i.e. 16 consecutive 16-byte slots taken mod 16 -- all 16 distinct in every group
//     ({0-3,12-15,4-11} and {4-11,0-3,12-15}) with no swizzle.  Packed row-major rows of 160 B (10 slots) are 2-way conflicted
//     as they stand and under every rotation of the chunk index by a function of the row that was tried, and the d64 XOR
//     (chunk ^ f(row), f < 8) leaves a 10-chunk row.  A glds16 instruction fills one plane of one tile
//     (64 lanes = 64 rows), so each row stages exactly D/8 chunks and the pad plane (D = 104: plane 13) is never written by DMA.
//   V^T image: [DV rows d][64 keys = 128 B], chunk swizzle attn_vswz: the layout both kernels share (the row length is 64 keys
//     at any D), conflict-free for its reads.
// LDS: 2 x (DK/8 KiB + DV/8 KiB) = 44 KiB at D = 80, 60 KiB at D = 104 (static; below the 64 KiB that needs an attribute).
//
// DESIGN 5.8 rule: no cross-lane exchange downstream of a per-lane-guarded load.  Every load here is unconditional from a clamped
// address (query row, key row, V^T column chunk, Q pad); the cross-half row maximum / row sum use v_permlane32_swap.
#include "attn_geo.h"

namespace {

using HdSeg = iir::AttnSeg;
using HdGeo = iir::AttnGeo;       // (c is 1 when Q is pre-scaled: see iir_attention_f16)
using iir::attn_vswz;
constexpr int KT = iir::ATTN_KT;

template <int D> struct HdShape {
    static constexpr int KS = (D + 15) / 16;        // k-steps of S^T = K . Q^T
    static constexpr int KC = 2 * KS;               // K image planes (16-byte chunks of a padded row)
    static constexpr int DC = D / 8;                // planes / V^T row groups staged from memory
    static constexpr int NDB = (D + 31) / 32;       // 32-row blocks of O^T
    static constexpr int DV = 32 * NDB;             // V^T image rows
    static constexpr int KBYTES = KC * KT * 16;     // one K tile image
    static constexpr int VBYTES = DV * 128;         // one V^T tile image
    static_assert(D % 8 == 0 && DC <= KC, "head_dim must be a multiple of 8");
};

template <int D>
__global__ __launch_bounds__(256) void attn_hd_kernel(const HdGeo g) {
    using S = HdShape<D>;
    __shared__ __attribute__((aligned(16))) char smem[2 * (S::KBYTES + S::VBYTES)];
    char* Ks = smem;                        // [2][KC planes][64 rows][16 B]
    char* Vs = smem + 2 * S::KBYTES;        // [2][DV rows][128 B]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, hh = lane >> 5;
    const int lin = iir::attn_lin(gridDim.x);
    const int pair = lin / g.qtiles;
    const int h = pair % g.heads, b = pair / g.heads;
    const int q0 = (lin % g.qtiles) * 128 + wave * 32;
    const int qq = q0 + qi;

    // zero the pad of both ring slots once: K planes [DC, KC) and V^T rows [D, DV) (ordered by the first tile's barrier)
    {
        constexpr int kpad = (S::KC - S::DC) * KT * 16, vpad = (S::DV - D) * 128;
        for (int i = tid * 16; i < kpad; i += 256 * 16)
#pragma unroll
            for (int s = 0; s < 2; ++s) *(f32x4*)(Ks + s * S::KBYTES + S::DC * KT * 16 + i) = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int i = tid * 16; i < vpad; i += 256 * 16)
#pragma unroll
            for (int s = 0; s < 2; ++s) *(f32x4*)(Vs + s * S::VBYTES + D * 128 + i) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // Q fragments: B operand of S^T = K.Q^T -- lane (q, hh) holds d = 16*ks + 8*hh + [0,8); the pad half is zeroed in registers.
    // (Q as given: the scores are scaled by g.c in the softmax, as in the d64 kernel's first generation.)
    f16x8 qf[S::KS];
    {
        const int q = qq < g.Tq ? qq : g.Tq - 1;
        const f16* qp = g.Q + (long)b * g.qbs + (long)q * g.ldq + h * D;
#pragma unroll
        for (int ks = 0; ks < S::KS; ++ks) {
            const bool pad = 16 * ks + 8 * hh >= D;                 // (D = 104: ks = 6, hh = 1)
            const f16x8 v = *(const f16x8*)(qp + (pad ? 16 * ks : 16 * ks + 8 * hh));     // clamped into the own head
            qf[ks] = pad ? (f16x8){0, 0, 0, 0, 0, 0, 0, 0} : v;
        }
    }

    f32x16 oout[S::NDB];
#pragma unroll
    for (int i = 0; i < S::NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oout[i][r] = 0.f;

    for (int sg = 0; sg < g.nseg; ++sg) {
        const HdSeg s = g.seg[sg];
        const f16* kbase = s.K + (long)b * s.kbs + h * D;
        const f16* vbase = s.Vt + (long)(h * D) * s.ldvt + (long)b * s.vbs;
        const int ntiles = (s.Tkv + KT - 1) / KT;
        const int tpad = (s.Tkv + 7) & ~7;   // contract: Vt rows readable and finite on [0, tpad)

        // one tile: DC K planes (one glds16 each: lane = LDS row) and DC V^T row groups (8 rows each), spread over the 4 waves
        auto stage = [&](int t, int buf) {
            {
                const f16* src = kbase + (long)iir::attn_krow_key(t, lane, s.Tkv) * s.ldk;      // LDS row = lane
                for (int c = wave; c < S::DC; c += 4) glds16(src + c * 8, Ks + buf * S::KBYTES + c * KT * 16);
            }
            const int srow = lane >> 3, spos = lane & 7;
            for (int i = wave; i < S::DC; i += 4) {
                const int d = i * 8 + srow;
                glds16(vbase + (long)d * s.ldvt + iir::attn_vt_col(t, spos, d, tpad), Vs + buf * S::VBYTES + i * 8 * 128);
            }
        };

        float m = -INFINITY, l = 0.f;
        f32x16 o[S::NDB];
#pragma unroll
        for (int i = 0; i < S::NDB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] = 0.f;

        stage(0, 0);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();

        for (int t = 0; t < ntiles; ++t) {
            const int buf = t & 1;
            if (t + 1 < ntiles) stage(t + 1, buf ^ 1);
            const char* kt = Ks + buf * S::KBYTES;
            const char* vt = Vs + buf * S::VBYTES;

            // ---- S^T = K . Q^T (2 blocks of 32 LDS rows); k-step ks, lane half hh reads plane 2*ks + hh
            f32x16 sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const char* krow = kt + (kb * 32 + qi) * 16;
#pragma unroll
                for (int ks = 0; ks < S::KS; ++ks) {
                    const f16x8 kf = *(const f16x8*)(krow + (2 * ks + hh) * KT * 16);
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        kf, qf[ks], ks ? sacc[kb] : (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0);
                }
            }
            // ---- masks: keys past the segment (last tile) and, causal, keys after the query.  Register r of block kb, lane half hh
            //      is key 32*kb + 16*(r >> 3) + 8*hh + (r & 7) of the tile.
            if ((t + 1) * KT > s.Tkv || (g.causal && (t + 1) * KT > q0)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = t * KT + kb * 32 + 16 * (r >> 3) + 8 * hh + (r & 7);
                        if (key >= s.Tkv || (g.causal && key > qq)) sacc[kb][r] = -INFINITY;
                    }
            }
            // ---- online softmax (base 2); key 0 is visible to every query, so m is finite after the first tile
            float mx = sacc[0][0];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
            const float m_new = fmaxf(m, iir::xhalf_max(mx) * g.c);
            if (__any(m_new > m)) {
                const float alpha = __builtin_amdgcn_exp2f(m - m_new);
                l *= alpha;
#pragma unroll
                for (int i = 0; i < S::NDB; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
                m = m_new;
            }
            float lsum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][r], g.c, -m));
                    sacc[kb][r] = p;
                    lsum += p;
                }
            l += lsum;

            // ---- O^T += V^T . P^T: k-step (kb, sp) covers keys 32kb + 16sp + [0,16); lane half hh holds keys + 8hh + [0,8)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int sp = 0; sp < 2; ++sp) {
                    f16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (f16)sacc[kb][8 * sp + j];
                    const int chunk = kb * 4 + sp * 2 + hh;
#pragma unroll
                    for (int db = 0; db < S::NDB; ++db) {
                        const int d = db * 32 + qi;
                        const f16x8 vf = *(const f16x8*)(vt + d * 128 + ((chunk ^ attn_vswz(d)) * 16));
                        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[db], 0, 0, 0);
                    }
                }
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
        }
        const float inv = 1.0f / iir::xhalf_sum(l);
#pragma unroll
        for (int i = 0; i < S::NDB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oout[i][r] += o[i][r] * inv;
    }

    // ---- store d < D (lane mapping: attn_o_col; D % 8 == 0: whole groups)
    if (qq < g.Tq) {
        f16* op = g.O + (long)b * g.obs + (long)qq * g.ldo + h * D;
#pragma unroll
        for (int db = 0; db < S::NDB; ++db)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                if (db * 32 + gq * 8 >= D) continue;
                *(f16x4*)(op + iir::attn_o_col(db, gq, hh)) = iir::attn_o_quad(oout[db], gq);
            }
    }
}

}  // namespace

extern "C" int iir_attention_f16(const iir_attn_desc* a, int32_t head_dim, void* stream) {
    if (head_dim == 64) return iir_attention_d64_f16(a, stream);         // (which checks `a` itself)
    if (head_dim != 80 && head_dim != 104) return IIR_EINVAL;
    if (!iir::attn_desc_ok(a) || a->o_fp8) return IIR_EINVAL;
    (void)hipGetLastError();
    HdGeo g = iir::attn_geo(a, a->batch);
    if (g.qpre) g.c = 1.0f;            // this kernel scales the scores by c in the softmax: a pre-scaled Q is used as it stands
    const dim3 grid(g.n_attn);
    if (head_dim == 80) iir_launch(attn_hd_kernel<80>, grid, dim3(256), 0, (hipStream_t)stream, g);
    else iir_launch(attn_hd_kernel<104>, grid, dim3(256), 0, (hipStream_t)stream, g);
    return iir_launch_status();
}
