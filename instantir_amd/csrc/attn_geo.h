// What attention.hip (head dim 64) and attention_hd.hip (80 / 104) share: the launch geometry and its fill from `iir_attn_desc`,
// the argument check of the exported entries, and the device pieces both kernels use in the same form -- workgroup order, staging
// order of a K tile, V^T swizzle, cross-half reductions, output lane mapping.  The tile bodies differ on purpose and stay there.
#pragma once
#include "common.h"
#include "../../include/instantir_hip.h"

namespace iir {

constexpr int ATTN_KT = 64;   // keys per tile

struct AttnSeg { const f16* K; long ldk, kbs; const f16* Vt; long ldvt, vbs; int Tkv; };
struct AttnGeo {
    const f16* Q; long ldq, qbs;
    f16* O; long ldo, obs; int o_fp8;      // o_fp8: O is a byte matrix of fp8-E4M3 (ldo / obs in bytes)
    int Tq, nseg;
    int qtiles, heads;    // query tiles per (batch, head)
    int causal;            // mask keys with index > query index (CLIP text encoders)
    int qpre;              // Q already multiplied by c
    float c;   // softmax scale * log2(e)
    AttnSeg seg[2];
    int n_attn;            // identity form: workgroups [0, n_attn) attend (batch rows below ident_from), the rest copy V
    int ident_from;
};

// What every entry refuses (each adds its own refusals); no HIP call.
static inline bool attn_desc_ok(const iir_attn_desc* a) {
    if (!a || !a->Q || !a->O || a->nseg < 1 || a->nseg > 2) return false;
    if (a->Tq <= 0 || a->heads <= 0 || a->batch <= 0) return false;
    if (a->ldq % 8 || a->ldo % 4) return false;
    for (int i = 0; i < a->nseg; ++i) {
        const iir_attn_kv* s = &a->kv[i];
        if (!s->K || !s->Vt || s->Tkv <= 0 || s->ldk % 8 || s->ldvt % 8 || s->vt_batch_stride % 8) return false;
    }
    return true;
}

// Geometry of a checked descriptor.  Batch rows [0, attn_batch) attend (all of them but in the identity form).
static inline AttnGeo attn_geo(const iir_attn_desc* a, int attn_batch) {
    AttnGeo g{};
    g.Q = (const f16*)a->Q; g.ldq = a->ldq; g.qbs = a->q_batch_stride;
    g.O = (f16*)a->O; g.ldo = a->ldo; g.obs = a->o_batch_stride; g.o_fp8 = a->o_fp8 != 0;
    g.Tq = a->Tq; g.nseg = a->nseg;
    g.c = a->scale * 1.4426950408889634f;
    g.qpre = a->q_prescaled;
    for (int i = 0; i < a->nseg; ++i) {
        const iir_attn_kv* s = &a->kv[i];
        g.seg[i] = AttnSeg{(const f16*)s->K, s->ldk, s->k_batch_stride, (const f16*)s->Vt, s->ldvt, s->vt_batch_stride, s->Tkv};
    }
    g.qtiles = (a->Tq + 127) / 128;
    g.heads = a->heads;
    g.causal = a->causal;
    g.n_attn = a->heads * attn_batch * g.qtiles;
    g.ident_from = attn_batch;
    return g;
}

// XCD-aware placement: workgroups b, b+8, ... share an XCD, and XCD x gets a contiguous run of the (batch, head)-major order
// of the `nwg` attending workgroups (neighbouring query tiles of a pair read the same K / V^T through one L2).
__device__ __forceinline__ int attn_lin(int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = blockIdx.x & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
}

// Key staged into LDS row rho of tile t.  Row rho holds key pi(rho) = rho with bits 2 and 3 swapped: accumulator row
// (r&3) + 8*(r>>2) + 4*hh of the score MFMA then is key 16*(r>>3) + 8*hh + (r&7) -- a lane's 8 scores of a k-step are 8
// CONSECUTIVE keys.  Rows past the end of the segment repeat its last key (masked by the tile body).
__device__ __forceinline__ int attn_krow_key(int t, int rho, int Tkv) {
    const int key = t * ATTN_KT + ((rho & ~12) | ((rho & 4) << 1) | ((rho & 8) >> 1));
    return key >= Tkv ? Tkv - 1 : key;
}

// V^T image: [rows d][64 keys = 128 B], 16-byte chunk c of row d stored at chunk c ^ attn_vswz(d) (conflict-free fragment reads)
__device__ __forceinline__ int attn_vswz(int d) { return (d >> 1) & 7; }
// First key column fetched by the lane that fills LDS chunk `spos` of row d, tile t.  Contract: V^T rows are readable and finite
// on [0, tpad); a chunk wholly past that reads column 0 instead (all its keys are masked).
__device__ __forceinline__ int attn_vt_col(int t, int spos, int d, int tpad) {
    const int kcol = t * ATTN_KT + (spos ^ attn_vswz(d)) * 8;
    return kcol >= tpad ? 0 : kcol;
}

// Row maximum / row sum across the two lane halves (keys 8*hh + [0,8) of a k-step): v_permlane32_swap, VALU, no LDS.
__device__ __forceinline__ float xhalf_max(float v) {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// Output: lane (q, hh) holds d = 32*db + 8*gq + 4*hh + [0,4) of its query in registers 4*gq .. 4*gq+3 of accumulator block db.
__device__ __forceinline__ int attn_o_col(int db, int gq, int hh) { return db * 32 + gq * 8 + hh * 4; }
__device__ __forceinline__ f16x4 attn_o_quad(const f32x16& o, int gq) {
    f16x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (f16)o[4 * gq + j];
    return v;
}

}  // namespace iir
