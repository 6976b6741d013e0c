// DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity", TPAMI 2020) around the MFMA conv:
// what lies between the thirteen 3x3 convs of VGG-16 `features` in DISTS and is not LPIPS's.  No reference counterpart; contract
// in include/instantir_hip.h (iir_dists_l2pool, iir_dists_stats, iir_dists_image_stats) and DESIGN.md section 7 "DISTS".
// Compiled with -ffp-contract=off: nothing is fused that is not written as fma.
//
// The contract in short.  Stage 0 is the raw image (fp32, never rounded to a 16-bit type); stage 1 is convs 0, 2 of VGG-16 on
// (x - mean) / std (iir_lpips_prep with shift = 2 mean - 1, scale = 2 std); stages 2..5 apply L2 pooling to the stage before
// and then convs (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28), a ReLU after every conv.  The L2 pool is, per channel,
//     out(i, j) = sqrt(sum_{di, dj in -1..1} g[di] g[dj] x(2i + di, 2j + dj)^2 + 1e-12),   g = (1/4, 1/2, 1/4),
// zero padding, stride 2, pad 1: output sides ceil(H / 2), ceil(W / 2).  Each of the 3 + 64 + 128 + 256 + 512 + 512 channels is
// compared as SSIM compares: from {sum a, sum b, sum a^2, sum b^2, sum ab} over the stage's pixels the host forms means,
// variances and the covariance, S1 = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1), S2 = (2 s_ab + c2) / (s_a^2 + s_b^2 + c2),
// c1 = c2 = 1e-6, and DISTS = 1 - sum_c (alpha_c S1_c + beta_c S2_c) / (sum alpha + sum beta)  (instantir_amd/dists.py).
//
// Two kernels and a final pass on NHWC 16-bit rows (fp16 or bf16 by `dtype`); both read the stage's last conv's PRE-activation
// rows and apply the ReLU on read, so no relu launch precedes them:
//   l2pool  one thread owns 8 channels (one 16-byte load per tap) of one output pixel and reads its nine inputs, all issued
//           before the first use.  fp32: squares of 16-bit values and the power-of-two weights are exact, so the roundings are
//           the eight additions (raster order of the taps), the + 1e-12, the square root and the store.  A tap outside the image
//           is loaded from the clamped address and multiplied by 0.
//   stats   the five raw sums per channel, fp64 from the first element: a 16-bit (or fp32) value converts exactly, the product
//           of two 16-bit values is exact in fp64, so fma(a, b, s) rounds once, as s + a * b does.  A lane keeps CH channels x 5
//           accumulators over the pixels it strides through (CH = 8: 80 VGPRs); the NT / chunks lanes of a channel group add
//           in LDS by a fixed halving tree over the group index, one statistic at a time (16 KB); the workgroup writes its
//           partial to ws; the final launch adds the partials of a column as 8 strided sequences in index order and those
//           eight in index order.  The split into workgroups depends on H * W and C alone: no atomics, equal inputs give equal
//           bits, and `pairs` = 2 gives each pair the bits of its own launch.
//   image   the same reduction (one template) for stage 0, reading the two image sources: three channels per lane.
// Every global load is unconditional from a clamped address and masked in registers; only stores are guarded.  64-bit offsets.
#include "image_common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_C = IIR_LPIPS_MAX_C;
constexpr int STATS = IIR_DISTS_STATS;
constexpr int FINAL_COLS = 32, FINAL_SLICES = NT / FINAL_COLS;
static_assert(STATS == 5, "sum a, sum b, sum a^2, sum b^2, sum ab");

// ---- L2 pooling ------------------------------------------------------------------------------------------------------------
// grid ceil(images * OH * OW * chunks / NT); a thread owns 8 channels of one output pixel
template <typename E>
__global__ __launch_bounds__(NT) void dists_l2pool_kernel(const E* x, long ldx, int H, int W, int OH, int OW, int chunks, long total, E* out,
                                                          long ldo) {
    const long t = (long)blockIdx.x * NT + threadIdx.x;
    const long tc = min(t, total - 1);
    const long opix = tc / chunks;
    const int col = (int)(tc - opix * chunks) * 8;
    const long img = opix / ((long)OH * OW);
    const long r = opix - img * ((long)OH * OW);
    const int oy = (int)(r / OW), ox = (int)(r - (long)oy * OW);
    float v[9][8], wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int di = k / 3 - 1, dj = k % 3 - 1;
        const int y = 2 * oy + di, xx = 2 * ox + dj;
        const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
        wt[k] = in ? (di == 0 ? 0.5f : 0.25f) * (dj == 0 ? 0.5f : 0.25f) : 0.0f;
        const long row = (img * H + min(max(y, 0), H - 1)) * W + min(max(xx, 0), W - 1);
        load8(x + row * ldx + col, v[k]);
    }
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float a = relu_f(v[k][i]);
            const float term = wt[k] * (a * a);
            s = k == 0 ? term : s + term;
        }
        o[i] = sqrtf(s + 1e-12f);
    }
    if (t < total) store8(out + opix * ldo + col, o);
}

// ---- the five sums ---------------------------------------------------------------------------------------------------------
struct StatsGeo {
    long pixels;      // H * W: the pixels of one image
    long b_off;       // rows between image i and its b partner (16-bit rows), unused by the image source
    int chunks;       // lanes per pixel: C / 8 for rows, 1 for an image
    int groups;       // NT / chunks: the pixels a workgroup reads at once
    int iters;        // pixels per lane
    int parts;        // workgroups per pair
    int cols;         // chunks * CH: the channels
};

// 16-bit NHWC rows, the ReLU on read
template <typename E> struct RowSrc {
    static constexpr int CH = 8;
    const E* x;
    long ldx, b_off;
    __device__ __forceinline__ void load(long pair, long pixels, long p, int chunk, float (&a)[CH], float (&b)[CH]) const {
        const long row = pair * pixels + p;
        load8(x + row * ldx + chunk * 8, a);
        load8(x + (row + b_off) * ldx + chunk * 8, b);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            a[i] = relu_f(a[i]);
            b[i] = relu_f(b[i]);
        }
    }
};

// the two image sources of stage 0: fp32 planar (N, 3, H, W) or uint8 interleaved (N, H, W, 3), x = u / 255 in fp32
struct ImgSrc {
    static constexpr int CH = 3;
    const void *a_, *b_;
    int u8;
    __device__ __forceinline__ void load(long n, long pixels, long p, int, float (&a)[CH], float (&b)[CH]) const {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (u8) {
                a[c] = (float)((const uint8_t*)a_)[(n * pixels + p) * 3 + c] / 255.0f;
                b[c] = (float)((const uint8_t*)b_)[(n * pixels + p) * 3 + c] / 255.0f;
            } else {
                a[c] = ((const float*)a_)[(n * 3 + c) * pixels + p];
                b[c] = ((const float*)b_)[(n * 3 + c) * pixels + p];
            }
        }
    }
};

// grid (parts, pairs), NT threads.  Lane (grp, chunk) = (tid / chunks, tid % chunks) strides through the workgroup's
// groups * iters pixels; ws: double[pairs][parts][cols][STATS]
template <typename S> __global__ __launch_bounds__(NT) void dists_stats_kernel(const S src, const StatsGeo g, double* ws) {
    constexpr int CH = S::CH;
    __shared__ double red[NT][CH];
    const int tid = threadIdx.x;
    const int grp = tid / g.chunks, chunk = tid - grp * g.chunks;
    const bool lane_ok = grp < g.groups;
    const long pair = blockIdx.y;
    const long base = (long)blockIdx.x * g.groups * g.iters + min(grp, g.groups - 1);

    double acc[STATS][CH];
#pragma unroll
    for (int k = 0; k < STATS; ++k)
#pragma unroll
        for (int i = 0; i < CH; ++i) acc[k][i] = 0.0;

    for (int it = 0; it < g.iters; it += 2) {
        float a[2][CH], b[2][CH];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long p = base + (long)(it + u) * g.groups;
            ok[u] = lane_ok && it + u < g.iters && p < g.pixels;
            src.load(pair, g.pixels, min(p, g.pixels - 1), chunk, a[u], b[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const double da = ok[u] ? (double)a[u][i] : 0.0, db = ok[u] ? (double)b[u][i] : 0.0;
                acc[0][i] += da;
                acc[1][i] += db;
                acc[2][i] = fma(da, da, acc[2][i]);
                acc[3][i] = fma(db, db, acc[3][i]);
                acc[4][i] = fma(da, db, acc[4][i]);
            }
        }
    }

    // groups -> one, a fixed halving tree over the group index, one statistic at a time
    int top = 1;
    while (top < g.groups) top *= 2;
    double* dst = ws + ((pair * g.parts + blockIdx.x) * g.cols + (long)chunk * CH) * STATS;
#pragma unroll
    for (int k = 0; k < STATS; ++k) {
#pragma unroll
        for (int i = 0; i < CH; ++i) red[tid][i] = acc[k][i];
        __syncthreads();
        for (int o = top / 2; o > 0; o >>= 1) {
            if (grp < o && grp + o < g.groups) {
#pragma unroll
                for (int i = 0; i < CH; ++i) red[tid][i] += red[tid + o * g.chunks][i];
            }
            __syncthreads();
        }
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < CH; ++i) dst[i * STATS + k] = red[tid][i];
        }
        __syncthreads();
    }
}

// grid (ceil(cols * STATS / FINAL_COLS), pairs), NT threads: column j of a pair's `parts` rows of `width` partial sums; slice s
// adds rows s, s + FINAL_SLICES, ... in index order, thread (0, j) the slices in index order
__global__ __launch_bounds__(NT) void dists_final_kernel(const double* ws, int parts, int width, double* out) {
    __shared__ double r[FINAL_SLICES][FINAL_COLS];
    const int j = threadIdx.x % FINAL_COLS, s = threadIdx.x / FINAL_COLS;
    const int col = blockIdx.x * FINAL_COLS + j;
    const int cc = min(col, width - 1);
    const double* p = ws + (long)blockIdx.y * parts * width + cc;
    double q = 0.0;
    for (int i = s; i < parts; i += FINAL_SLICES) q += p[(long)i * width];
    r[s][j] = q;
    __syncthreads();
    if (s == 0 && col < width) {
        double a = r[0][j];
#pragma unroll
        for (int k = 1; k < FINAL_SLICES; ++k) a += r[k][j];
        out[(long)blockIdx.y * width + col] = a;
    }
}

// the split of one pair's H * W pixels into workgroups: a function of the geometry alone.  A lane reads 8 .. 64 pixels, about
// 1024 workgroups per pair where the image allows it.
bool stats_plan(int pairs, int H, int W, int chunks, int ch, StatsGeo* g) {
    if (pairs <= 0 || pairs > 65535 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || chunks <= 0 || chunks > NT) return false;
    g->pixels = (long)H * W;
    g->b_off = (long)pairs * g->pixels;
    g->chunks = chunks;
    g->groups = NT / chunks;
    g->cols = chunks * ch;
    const long per = (long)g->groups * 1024;
    long iters = (g->pixels + per - 1) / per;
    iters = iters < 8 ? 8 : iters > 64 ? 64 : iters;
    g->iters = (int)iters;
    const long span = (long)g->groups * iters;
    const long parts = (g->pixels + span - 1) / span;
    if (parts * pairs > 0x7fffffffLL) return false;
    g->parts = (int)parts;
    return true;
}

int64_t stats_ws_bytes(const StatsGeo& g, int pairs) { return (int64_t)pairs * g.parts * g.cols * STATS * (int64_t)sizeof(double); }

template <typename S> void stats_launch(const S& src, const StatsGeo& g, int pairs, double* ws, double* out, hipStream_t s) {
    hipLaunchKernelGGL((dists_stats_kernel<S>), dim3((unsigned)g.parts, (unsigned)pairs), dim3(NT), 0, s, src, g, ws);
    const int width = g.cols * STATS;
    hipLaunchKernelGGL(dists_final_kernel, dim3((unsigned)((width + FINAL_COLS - 1) / FINAL_COLS), (unsigned)pairs), dim3(NT), 0, s,
                       (const double*)ws, g.parts, width, out);
}

}  // namespace

extern "C" int iir_dists_l2pool(const void* x, int64_t ldx, int32_t images, int32_t H, int32_t W, int32_t C, int32_t dtype, void* out, int64_t ldo,
                                void* stream) {
    if (!x || !out || ((uintptr_t)x | (uintptr_t)out) % 16) return IIR_EINVAL;
    if (images <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || C <= 0 || C % 8 || C > MAX_C) return IIR_EINVAL;
    if (ldx < C || ldx % 8 || ldo < C || ldo % 8) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, chunks = C / 8;
    const int64_t opix = (int64_t)images * OH * OW;
    if (opix > (0x7fffffffLL * NT) / chunks) return IIR_EINVAL;
    const int64_t total = opix * chunks, blocks = (total + NT - 1) / NT;
    if (overlap(x, (int64_t)images * H * W * ldx * 2, out, opix * ldo * 2)) return IIR_EINVAL;      // other windows are still to be read
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (dtype == IIR_DT_BF16)
        hipLaunchKernelGGL(dists_l2pool_kernel<bf16>, dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16*)x, (long)ldx, H, W, OH, OW, chunks,
                           (long)total, (bf16*)out, (long)ldo);
    else
        hipLaunchKernelGGL(dists_l2pool_kernel<f16>, dim3((unsigned)blocks), dim3(NT), 0, s, (const f16*)x, (long)ldx, H, W, OH, OW, chunks,
                           (long)total, (f16*)out, (long)ldo);
    return iir_launch_status();
}

extern "C" int64_t iir_dists_stats_workspace_bytes(int32_t pairs, int32_t H, int32_t W, int32_t C) {
    StatsGeo g;
    if (C <= 0 || C % 8 || C > MAX_C || !stats_plan(pairs, H, W, C / 8, 8, &g)) return -1;
    return stats_ws_bytes(g, pairs);
}

extern "C" int iir_dists_stats(const void* x, int64_t ldx, int32_t pairs, int32_t H, int32_t W, int32_t C, int32_t dtype, void* ws,
                               int64_t ws_bytes, double* out, void* stream) {
    StatsGeo g;
    if (C <= 0 || C % 8 || C > MAX_C || !stats_plan(pairs, H, W, C / 8, 8, &g)) return IIR_EINVAL;
    if (!x || !ws || !out) return IIR_EINVAL;
    if (dtype != IIR_DT_F16 && dtype != IIR_DT_BF16) return IIR_EINVAL;
    if (ldx < C || ldx % 8 || (uintptr_t)x % 16) return IIR_EINVAL;
    if (((uintptr_t)ws | (uintptr_t)out) & 7) return IIR_EINVAL;
    if (ws_bytes < stats_ws_bytes(g, pairs)) return IIR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (dtype == IIR_DT_BF16) stats_launch(RowSrc<bf16>{(const bf16*)x, (long)ldx, g.b_off}, g, pairs, (double*)ws, out, s);
    else stats_launch(RowSrc<f16>{(const f16*)x, (long)ldx, g.b_off}, g, pairs, (double*)ws, out, s);
    return iir_launch_status();
}

extern "C" int64_t iir_dists_image_stats_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    StatsGeo g;
    if (!stats_plan(N, H, W, 1, 3, &g)) return -1;
    return stats_ws_bytes(g, N);
}

extern "C" int iir_dists_image_stats(const void* src_a, const void* src_b, int32_t src_u8, int32_t N, int32_t H, int32_t W, void* ws,
                                     int64_t ws_bytes, double* out, void* stream) {
    StatsGeo g;
    if (!stats_plan(N, H, W, 1, 3, &g)) return IIR_EINVAL;
    if (!src_a || !src_b || !ws || !out) return IIR_EINVAL;
    if (!src_u8 && (((uintptr_t)src_a | (uintptr_t)src_b) % 4)) return IIR_EINVAL;
    if (((uintptr_t)ws | (uintptr_t)out) & 7) return IIR_EINVAL;
    if (ws_bytes < stats_ws_bytes(g, N)) return IIR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    stats_launch(ImgSrc{src_a, src_b, (int)(src_u8 != 0)}, g, N, (double*)ws, out, s);
    return iir_launch_status();
}
