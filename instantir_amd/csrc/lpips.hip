// LPIPS v0.1 (net = vgg) around the MFMA conv: what the thirteen 3x3 convs of VGG-16 `features` do not do themselves.  The
// reference builds `lpips.LPIPS(net='vgg')` at losses/losses.py:81-95; contract in include/instantir_hip.h (iir_lpips_prep,
// iir_relu_f16, iir_lpips_tap) and DESIGN.md section 7 "LPIPS".  The summation orders are image_common.h's.  Compiled with
// -ffp-contract=off: nothing is fused that is not written as fmaf.
//
// Three kernels on NHWC 16-bit rows (fp16 or bf16 by `dtype`, fp32 arithmetic):
//   prep   image (uint8 interleaved or fp32 planar, [0, 1]) -> the scaling layer's output as rows of IIR_LPIPS_CPAD channels,
//          three real and the rest zero: the input of the first conv.  u / 255 is one fp32 division for a uint8 source, the
//          affine runs in fp64 and is rounded once to fp32 and once to the 16-bit type.
//   relu   in place over a (rows, C) matrix: the eight convs that are neither tapped nor pooled.  On the bits: a value with
//          the sign bit that is not a NaN becomes +0, every other bit pattern stays.
//   tap    the pre-activation rows of a tapped conv for the `a` half and the `b` half of a stacked batch -> the LPIPS distance
//          of the tap and, from the same registers, the 2x2 max-pooled ReLU output both halves go on with.
// The tap's mapping.  A lane owns 8 channels (one 16-byte load); LP = the power of two >= C / 8 lanes own a pixel, so C <= 512
// fits one wave and a pixel's three channel sums (|a|^2, |b|^2, sum_c w_c (a^ - b^)^2) are butterflies over LP lanes, whose
// result is the same bits in every lane.  Such a lane group owns one 2x2 quad of one image pair: eight loads, all issued
// before the first use, then per pixel ReLU, the two norms, d(p), and a running channel-wise maximum that becomes the pooled
// row when the quad is whole (floor semantics: an odd last row or column is scored and not pooled).  The group's lane 0 holds
// the quad's sum of d in fp32 (four terms, fixed order) and writes the map; the workgroup adds its groups in fp64 (wave
// butterflies, then the four waves in order) and leaves one partial; a second launch adds a pair's partials in fp64 in index
// order (256 strided sequences, then a fixed tree) and divides by H * W.
// Every global load is unconditional from a clamped address and masked in registers; only stores are guarded.  No atomics, no
// scratch: equal inputs give equal bits.
#include "image_common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int NT = 256;
constexpr int CPAD = IIR_LPIPS_CPAD;
constexpr int MAX_C = IIR_LPIPS_MAX_C;
static_assert(CPAD % 8 == 0 && MAX_C == 64 * 8, "one wave holds a pixel");

// grid ceil(N * H * W * (CPAD / 8) / NT); a thread owns 8 of a pixel's CPAD output channels
template <typename E>
__global__ __launch_bounds__(NT) void lpips_prep_kernel(const void* src, int u8, long pixels, long HW, const double* affine, E* out, long ldo) {
    const long t = (long)blockIdx.x * NT + threadIdx.x;
    const long px = min(t / (CPAD / 8), pixels - 1);
    const int chunk = (int)(t % (CPAD / 8));
    const long n = px / HW, r = px - n * HW;
    float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = u8 ? (float)((const uint8_t*)src)[px * 3 + c] / 255.0f : ((const float*)src)[(n * 3 + c) * HW + r];
        const double s = ((2.0 * (double)x - 1.0) - affine[c]) / affine[3 + c];
        v[c] = chunk == 0 ? (float)s : 0.0f;
    }
    if (t / (CPAD / 8) < pixels) store8(out + px * ldo + chunk * 8, v);
}

// grid ceil(rows * (C / 8) / NT); a thread owns 8 elements
__global__ __launch_bounds__(NT) void relu16_kernel(uint16_t* x, long ld, long rows, int chunks, unsigned inf_bits) {
    const long t = (long)blockIdx.x * NT + threadIdx.x, total = rows * chunks;
    const long tc = min(t, total - 1);
    const long row = tc / chunks;
    uint4* p = (uint4*)(x + row * ld + (tc - row * chunks) * 8);
    uint4 q = *p;
    unsigned* w = (unsigned*)&q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = w[i] & 0xffffu, hi = w[i] >> 16;
        const unsigned l2 = ((lo & 0x8000u) && (lo & 0x7fffu) <= inf_bits) ? 0u : lo;
        const unsigned h2 = ((hi & 0x8000u) && (hi & 0x7fffu) <= inf_bits) ? 0u : hi;
        w[i] = l2 | (h2 << 16);
    }
    if (t < total) *p = q;
}

template <int LP> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct TapGeo {
    int H, W, C, chunks;      // the tap's extent; chunks = C / 8
    int qh, qw;               // quads per axis, the odd remainder included
    int ph, pw;               // pooled extent (floor)
    long quads;               // qh * qw
    long img_rows;            // H * W
    long b_off;               // rows between the a half and the b half: pairs * H * W
    long pb_off;              // the same in the pooled buffer: pairs * ph * pw
};

// grid (ceil(quads / (NT / LP)), pairs), NT threads
template <typename E, int LP>
__global__ __launch_bounds__(NT) void lpips_tap_kernel(const E* x, long ldx, const TapGeo g, const float* lin_w, float* dmap, E* pooled, long ldp,
                                                       double* ws) {
    __shared__ double red[1][NT / 64];
    constexpr int G = NT / LP;
    const int tid = threadIdx.x, lane = tid % LP;
    const long pair = blockIdx.y;
    const long quad = (long)blockIdx.x * G + tid / LP;
    const bool quad_ok = quad < g.quads;
    const long qc = min(quad, g.quads - 1);
    const int qy = (int)(qc / g.qw), qx = (int)(qc - (long)qy * g.qw);
    const bool lane_ok = lane < g.chunks;
    const int col = min(lane, g.chunks - 1) * 8;

    float w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = lane_ok ? lin_w[col + i] : 0.0f;

    float a[4][8], b[4][8];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * qy + (k >> 1), xx = 2 * qx + (k & 1);
        live[k] = quad_ok && y < g.H && xx < g.W;
        const long row = pair * g.img_rows + (long)min(y, g.H - 1) * g.W + min(xx, g.W - 1);
        load8(x + row * ldx + col, a[k]);
        load8(x + (row + g.b_off) * ldx + col, b[k]);
    }

    float ma[8], mb[8], dq = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ma[i] = mb[i] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[k][i] = lane_ok ? relu_f(a[k][i]) : 0.0f;
            b[k][i] = lane_ok ? relu_f(b[k][i]) : 0.0f;
            sa = fmaf(a[k][i], a[k][i], sa);
            sb = fmaf(b[k][i], b[k][i], sb);
            ma[i] = a[k][i] > ma[i] ? a[k][i] : ma[i];
            mb[i] = b[k][i] > mb[i] ? b[k][i] : mb[i];
        }
        sa = group_sum<LP>(sa);
        sb = group_sum<LP>(sb);
        const float ra = 1.0f / (sqrtf(sa) + 1e-10f), rb = 1.0f / (sqrtf(sb) + 1e-10f);
        float d = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float e = a[k][i] * ra - b[k][i] * rb;
            d = fmaf(w[i], e * e, d);
        }
        d = group_sum<LP>(d);
        if (live[k] && lane == 0 && dmap) dmap[pair * g.img_rows + (long)(2 * qy + (k >> 1)) * g.W + 2 * qx + (k & 1)] = d;
        dq += live[k] ? d : 0.0f;
    }
    if (pooled && quad_ok && lane_ok && qy < g.ph && qx < g.pw) {
        const long prow = (pair * g.ph + qy) * g.pw + qx;
        store8(pooled + prow * ldp + col, ma);
        store8(pooled + (prow + g.pb_off) * ldp + col, mb);
    }
    block_sum_stage(red, lane == 0 ? (double)dq : 0.0);
    __syncthreads();
    if (tid == 0) ws[pair * gridDim.x + blockIdx.x] = block_sum(red[0]);
}

// grid (pairs), NT threads: ws holds `parts` partial sums per pair
__global__ __launch_bounds__(NT) void lpips_final_kernel(const double* ws, int parts, double count, double* out) {
    __shared__ double r[1][NT];
    double sum[1];
    final_sum_f64<NT, 1>(ws + (long)blockIdx.x * parts, parts, r, sum);
    if (threadIdx.x == 0) out[blockIdx.x] = sum[0] / count;
}

int lanes_per_pixel(int C) {
    int lp = 1;
    while (lp * 8 < C) lp *= 2;
    return lp;
}

// the geometry checks of the tap, shared by both entries
bool tap_plan(int pairs, int H, int W, int C, TapGeo* g, int* lp, int64_t* parts) {
    if (pairs <= 0 || pairs > 65535 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || C <= 0 || C % 8 || C > MAX_C) return false;
    g->H = H; g->W = W; g->C = C; g->chunks = C / 8;
    g->qh = (H + 1) / 2; g->qw = (W + 1) / 2;
    g->ph = H / 2; g->pw = W / 2;
    g->quads = (long)g->qh * g->qw;
    g->img_rows = (long)H * W;
    g->b_off = (long)pairs * g->img_rows;
    g->pb_off = (long)pairs * g->ph * g->pw;
    *lp = lanes_per_pixel(C);
    const int G = NT / *lp;
    *parts = (g->quads + G - 1) / G;
    return *parts * pairs <= 0x7fffffffLL;
}

template <typename E, int LP>
void tap_launch(const void* x, int64_t ldx, const TapGeo& g, int pairs, int64_t parts, const float* lin_w, float* dmap, void* pooled, int64_t ldp,
                double* ws, hipStream_t s) {
    hipLaunchKernelGGL((lpips_tap_kernel<E, LP>), dim3((unsigned)parts, (unsigned)pairs), dim3(NT), 0, s, (const E*)x, (long)ldx, g, lin_w, dmap,
                       (E*)pooled, (long)ldp, ws);
}

template <typename E>
void tap_dispatch(int lp, const void* x, int64_t ldx, const TapGeo& g, int pairs, int64_t parts, const float* lin_w, float* dmap, void* pooled,
                  int64_t ldp, double* ws, hipStream_t s) {
    switch (lp) {
        case 1: return tap_launch<E, 1>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        case 2: return tap_launch<E, 2>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        case 4: return tap_launch<E, 4>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        case 8: return tap_launch<E, 8>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        case 16: return tap_launch<E, 16>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        case 32: return tap_launch<E, 32>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
        default: return tap_launch<E, 64>(x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, ws, s);
    }
}

}  // namespace

extern "C" int iir_lpips_prep(const void* src, int32_t src_u8, int32_t N, int32_t H, int32_t W, const double* affine, void* out, int64_t ldo,
                              int32_t dtype, void* stream) {
    if (!src || !affine || !out) return IIR_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return IIR_EINVAL;
    if (ldo < CPAD || ldo % 8 || (uintptr_t)out % 16 || (uintptr_t)affine % 8) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    if (!src_u8 && (uintptr_t)src % 4) return IIR_EINVAL;
    const int64_t pixels = (int64_t)N * H * W;
    const int64_t blocks = (pixels * (CPAD / 8) + NT - 1) / NT;
    if (blocks > 0x7fffffffLL) return IIR_EINVAL;
    if (overlap(src, pixels * 3 * (src_u8 ? 1 : 4), out, pixels * ldo * 2)) return IIR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (dtype == IIR_DT_BF16)
        hipLaunchKernelGGL(lpips_prep_kernel<bf16>, dim3((unsigned)blocks), dim3(NT), 0, s, src, (int)(src_u8 != 0), (long)pixels, (long)H * W, affine,
                           (bf16*)out, (long)ldo);
    else
        hipLaunchKernelGGL(lpips_prep_kernel<f16>, dim3((unsigned)blocks), dim3(NT), 0, s, src, (int)(src_u8 != 0), (long)pixels, (long)H * W, affine,
                           (f16*)out, (long)ldo);
    return iir_launch_status();
}

extern "C" int iir_relu_f16(void* x, int64_t ld, int64_t rows, int32_t C, int32_t dtype, void* stream) {
    if (!x || rows <= 0 || C <= 0 || C % 8 || ld < C || ld % 8 || (uintptr_t)x % 16) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    if (rows > (0x7fffffffLL * NT) / (C / 8)) return IIR_EINVAL;
    const int64_t blocks = (rows * (C / 8) + NT - 1) / NT;
    (void)hipGetLastError();
    hipLaunchKernelGGL(relu16_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (uint16_t*)x, (long)ld, (long)rows, C / 8,
                       dtype == IIR_DT_BF16 ? 0x7f80u : 0x7c00u);
    return iir_launch_status();
}

extern "C" int64_t iir_lpips_tap_workspace_bytes(int32_t pairs, int32_t H, int32_t W, int32_t C) {
    TapGeo g;
    int lp;
    int64_t parts;
    if (!tap_plan(pairs, H, W, C, &g, &lp, &parts)) return -1;
    return parts * pairs * (int64_t)sizeof(double);
}

extern "C" int iir_lpips_tap(const void* x, int64_t ldx, int32_t pairs, int32_t H, int32_t W, int32_t C, const float* lin_w, int32_t dtype,
                             float* dmap, void* pooled, int64_t ldp, void* ws, int64_t ws_bytes, double* out, void* stream) {
    TapGeo g;
    int lp;
    int64_t parts;
    if (!tap_plan(pairs, H, W, C, &g, &lp, &parts)) return IIR_EINVAL;
    if (!x || !lin_w || !ws || !out) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    if (ldx < C || ldx % 8 || (uintptr_t)x % 16 || (uintptr_t)lin_w % 4) return IIR_EINVAL;
    if (((uintptr_t)ws | (uintptr_t)out) & 7) return IIR_EINVAL;
    if (ws_bytes < parts * pairs * (int64_t)sizeof(double)) return IIR_EINVAL;
    if (dmap && (uintptr_t)dmap % 4) return IIR_EINVAL;
    const int64_t xbytes = 2 * g.b_off * ldx * 2;
    if (pooled) {
        if (g.ph <= 0 || g.pw <= 0 || ldp < C || ldp % 8 || (uintptr_t)pooled % 16) return IIR_EINVAL;
        if (overlap(x, xbytes, pooled, 2 * g.pb_off * ldp * 2)) return IIR_EINVAL;           // other quads' pixels are still to be read
    }
    if (dmap && overlap(x, xbytes, dmap, g.b_off * 4)) return IIR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (dtype == IIR_DT_BF16) tap_dispatch<bf16>(lp, x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, (double*)ws, s);
    else tap_dispatch<f16>(lp, x, ldx, g, pairs, parts, lin_w, dmap, pooled, ldp, (double*)ws, s);
    hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)pairs), dim3(NT), 0, s, (const double*)ws, (int)parts, (double)g.img_rows, out);
    return iir_launch_status();
}
