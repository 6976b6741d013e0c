// NIQE's device part: the natural-scene statistics of an image's luma at two scales, as per-block signed moments (no reference
// counterpart; contract in include/instantir_hip.h: iir_niqe_stats, and DESIGN.md section 7 "NIQE").  What is left -- the AGGD
// fit, the 36 features, the Gaussian model and the distance -- is a few hundred fp64 operations per block on the host
// (instantir_amd/niqe.py).  The pixel read, the luma, the rounding and the summation order are image_common.h's.  Compiled with
// -ffp-contract=off: the tap sums are written with fmaf, so they are fused by statement and nothing else is.
//
// Four launches.  niqe_grey_kernel writes the rounded grey value of every pixel of the block-grid image (the top-left
// 96 nbh x 96 nbw part of the cropped image) as an fp32 plane into the workspace; pixels outside that part are never read.
// niqe_half_kernel writes the half-size plane: MATLAB's antialiased bicubic at the factor 1/2 is a fixed 8-tap filter with
// symmetric indices, applied along y (exact in fp32: integers times k / 256) and then along x.  niqe_block_kernel<B>, once per
// scale (B = 96 on the full plane, 48 on the half-size one), gives a workgroup one block: it walks the block in strips of R
// rows, stages a strip with the 3-pixel halo of the 7 x 7 window in LDS (value minus 128, coordinates clamped to the plane, which
// IS the replicate padding the contract asks for at the edge of the block-grid image), filters x and x^2 along x into a second LDS
// image and along y from there, and keeps m = (x - mu) / (sigma + 1) of the whole block in LDS.  Then every thread forms the five
// maps (m and its four circularly shifted products) of its B * B / NT elements, sums each map's five statistics and sigma in fp32
// (at most 24 terms), goes to fp64, and the workgroup adds in a fixed order (wave butterflies, then the waves in order).
// Every global load is unconditional from a clamped address; only stores are guarded.  No atomics, no
// scratch: equal inputs give equal bits.
#include "image_common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int BLK = IIR_NIQE_BLOCK;                 // block side at scale 1; half of it at scale 2
constexpr int NSTAT = IIR_NIQE_STATS;
constexpr int WIN = 7, HALO = WIN - 1, RAD = 3;
constexpr int NT = 384;                             // a multiple of 96 and 48: a thread keeps its column
constexpr int NW = NT / 64;
constexpr int R = 16;                               // rows of a strip
constexpr int NPT = 256;                            // threads of the two pointwise launches
constexpr float PIVOT = 128.0f;
static_assert(NSTAT == 26, "5 maps x 5 statistics + sigma");

// g_j = exp(-(j - 3)^2 / (2 * (7/6)^2)) / sum, formed in fp64 and rounded to fp32
#define IIR_NIQE_TAPS {0x1.9b929ap-7f, 0x1.42e11cp-4f, 0x1.e5fb7cp-3f, 0x1.5edaccp-2f, 0x1.e5fb7cp-3f, 0x1.42e11cp-4f, 0x1.9b929ap-7f}
// MATLAB imresize(., 0.5), bicubic with antialiasing: exact in fp32
#define IIR_NIQE_HALF_TAPS {-3.0f / 256.0f, -9.0f / 256.0f, 29.0f / 256.0f, 111.0f / 256.0f, 111.0f / 256.0f, 29.0f / 256.0f, \
                            -9.0f / 256.0f, -3.0f / 256.0f}

struct Geo {
    int C, H, W;          // the source as stored
    int u8, crop;
    int hg, wg;           // the block-grid image: 96 nbh x 96 nbw
};

// grid (ceil(hg * wg / NPT), N), NPT threads: grey[n][y][x], rounded to the 8-bit grid
__global__ __launch_bounds__(NPT) void niqe_grey_kernel(const void* src, const Geo g, float* grey) {
    const int n = blockIdx.y;
    const long E = (long)g.hg * g.wg;
    const long e = (long)blockIdx.x * NPT + threadIdx.x, ec = min(e, E - 1);
    const int y = (int)(ec / g.wg), x = (int)(ec - (long)y * g.wg);
    const int sy = g.crop + y, sx = g.crop + x;
    const ImageSrc s = {src, g.u8, 0};
    const auto ch = [&](int c) { return image_load255(s, g.C, g.H, g.W, n, c, sy, sx); };
    const float v = round_u8(g.C == 3 ? luma_bt601(ch(0), ch(1), ch(2)) : ch(0));
    if (e < E) grey[n * E + e] = v;
}

__device__ __forceinline__ int sym(int i, int n) { return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i); }

// grid (ceil(hg / 2 * wg / 2 / NPT), N), NPT threads: half[n][oy][ox] from grey
__global__ __launch_bounds__(NPT) void niqe_half_kernel(const float* grey, int hg, int wg, float* half) {
    constexpr float taps[8] = IIR_NIQE_HALF_TAPS;
    const int n = blockIdx.y, hh = hg / 2, wh = wg / 2;
    const long E = (long)hh * wh;
    const long e = (long)blockIdx.x * NPT + threadIdx.x, ec = min(e, E - 1);
    const int oy = (int)(ec / wh), ox = (int)(ec - (long)oy * wh);
    const float* plane = grey + (long)n * hg * wg;
    int rows[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) rows[j] = sym(2 * oy - 3 + j, hg);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int xx = sym(2 * ox - 3 + i, wg);
        float col = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) col = fmaf(taps[j], plane[(long)rows[j] * wg + xx], col);
        acc = fmaf(taps[i], col, acc);
    }
    if (e < E) half[n * E + e] = acc;
}

template <int B> struct BlockLds {
    static constexpr int SW = B + HALO, SP = SW + 1, SR = R + HALO;
    float sa[SR * SP];           // the strip and its halo, minus 128
    float sx[2][SR * B];         // x-filtered x and x^2 over the strip's rows, the block's columns
    float sm[B * B];             // m of the whole block
    double red[NSTAT][NW];
};
static_assert(sizeof(BlockLds<BLK>) <= 64 * 1024, "static LDS");

// one map's five statistics of one value
__device__ __forceinline__ void tally(float v, int& cn, int& cp, float& qn, float& qp, float& ab) {
    const float q = v * v;
    cn += v < 0.0f ? 1 : 0;
    cp += v > 0.0f ? 1 : 0;
    qn += v < 0.0f ? q : 0.0f;
    qp += v > 0.0f ? q : 0.0f;
    ab += fabsf(v);
}

// grid (nbw, nbh, N), NT threads.  plane: fp32 (N, ph, pw) with ph = B nbh, pw = B nbw; out: this scale's double[nb][NSTAT] of
// image n at out + n * out_image_stride
template <int B> __global__ __launch_bounds__(NT) void niqe_block_kernel(const float* plane, int ph, int pw, double* out, long out_image_stride) {
    using L = BlockLds<B>;
    __shared__ L s;
    constexpr float taps[WIN] = IIR_NIQE_TAPS;
    constexpr int ROWS = NT / B, SW = L::SW, SP = L::SP, SR = L::SR;
    constexpr int STAGE = (SR * SW + NT - 1) / NT, PER = B * B / NT;
    static_assert(NT % B == 0 && R % ROWS == 0 && B % R == 0 && (B * B) % NT == 0 && B % ROWS == 0, "a thread keeps its column");
    const int tid = threadIdx.x, tx = tid % B, tr = tid / B;
    const int bx0 = blockIdx.x * B, by0 = blockIdx.y * B, n = blockIdx.z;
    const float* img = plane + (long)n * ph * pw;

    float ssig = 0.0f;
    for (int y0 = 0; y0 < B; y0 += R) {
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = tid + k * NT, ic = min(i, SR * SW - 1);
            const int ly = ic / SW, lx = ic - ly * SW;
            const int gy = min(max(by0 + y0 + ly - RAD, 0), ph - 1), gx = min(max(bx0 + lx - RAD, 0), pw - 1);
            const float v = img[(long)gy * pw + gx];
            if (i < SR * SW) s.sa[ly * SP + lx] = v - PIVOT;
        }
        __syncthreads();
        for (int ly = tr; ly < SR; ly += ROWS) {
            const float* ra = s.sa + ly * SP + tx;
            float m0 = 0.0f, m1 = 0.0f;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const float a = ra[j];
                m0 = fmaf(taps[j], a, m0);
                m1 = fmaf(taps[j], a * a, m1);
            }
            s.sx[0][ly * B + tx] = m0;
            s.sx[1][ly * B + tx] = m1;
        }
        __syncthreads();
        for (int y = tr; y < R; y += ROWS) {
            const float* c0 = s.sx[0] + y * B + tx;
            const float* c1 = s.sx[1] + y * B + tx;
            float mu = 0.0f, e2 = 0.0f;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                mu = fmaf(taps[j], c0[j * B], mu);
                e2 = fmaf(taps[j], c1[j * B], e2);
            }
            const float sigma = sqrtf(fabsf(e2 - mu * mu));
            const float x = s.sa[(y + RAD) * SP + tx + RAD];
            s.sm[(y0 + y) * B + tx] = (x - mu) / (sigma + 1.0f);
            ssig += sigma;
        }
        __syncthreads();           // sa and sx are restaged; sm is complete after the last strip
    }

    int cn[5] = {0, 0, 0, 0, 0}, cp[5] = {0, 0, 0, 0, 0};
    float qn[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, qp[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, ab[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int cl = tx == 0 ? B - 1 : tx - 1, cr = tx == B - 1 ? 0 : tx + 1;          // roll within the block
#pragma unroll 2
    for (int k = 0; k < PER; ++k) {
        const int r = tr + k * ROWS, ru = r == 0 ? B - 1 : r - 1;
        const float m = s.sm[r * B + tx];
        tally(m, cn[0], cp[0], qn[0], qp[0], ab[0]);
        tally(m * s.sm[r * B + cl], cn[1], cp[1], qn[1], qp[1], ab[1]);               // roll (0, 1)
        tally(m * s.sm[ru * B + tx], cn[2], cp[2], qn[2], qp[2], ab[2]);              // roll (1, 0)
        tally(m * s.sm[ru * B + cl], cn[3], cp[3], qn[3], qp[3], ab[3]);              // roll (1, 1)
        tally(m * s.sm[ru * B + cr], cn[4], cp[4], qn[4], qp[4], ab[4]);              // roll (1, -1)
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) block_sum_stage(s.red + 5 * q, cn[q], cp[q], qn[q], qp[q], ab[q]);
    block_sum_stage(s.red + NSTAT - 1, ssig);
    __syncthreads();
    if (tid < NSTAT) {
        const double a = block_sum(s.red[tid]);
        out[(long)n * out_image_stride + ((long)blockIdx.y * gridDim.x + blockIdx.x) * NSTAT + tid] = a;
    }
}

struct Args {
    int64_t N, C, H, W, crop_border;
};

struct Plan {
    int nbh, nbw, hg, wg;
    int64_t ws_bytes, out_bytes;
};

// the geometry checks of the contract, shared by both entries; the pointers are the caller's
bool plan(const Args& a, Plan* p) {
    if (a.N <= 0 || a.C <= 0 || a.H <= 0 || a.W <= 0 || a.H > 32768 || a.W > 32768) return false;
    if (a.C != 1 && a.C != 3) return false;
    if (a.crop_border < 0) return false;
    if (a.N > 65535) return false;                                                           // grid.y / grid.z
    const int64_t hc = a.H - 2 * a.crop_border, wc = a.W - 2 * a.crop_border;
    if (hc < BLK || wc < BLK) return false;
    p->nbh = (int)(hc / BLK); p->nbw = (int)(wc / BLK);
    p->hg = p->nbh * BLK; p->wg = p->nbw * BLK;
    const int64_t plane = (int64_t)p->hg * p->wg;
    if ((plane + NPT - 1) / NPT > 0x7fffffffLL) return false;
    p->ws_bytes = a.N * (plane + plane / 4) * (int64_t)sizeof(float);
    p->out_bytes = a.N * 2 * p->nbh * p->nbw * NSTAT * (int64_t)sizeof(double);
    return true;
}

}  // namespace

extern "C" int64_t iir_niqe_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop_border) {
    Plan p;
    if (!plan({N, C, H, W, crop_border}, &p)) return -1;
    return p.ws_bytes;
}

extern "C" int iir_niqe_stats(const void* src, int32_t src_u8, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop_border, void* ws,
                              int64_t ws_bytes, double* out, int64_t out_bytes, void* stream) {
    Plan p;
    if (!plan({N, C, H, W, crop_border}, &p)) return IIR_EINVAL;
    if (!src || !ws || !out) return IIR_EINVAL;
    if (((uintptr_t)ws | (uintptr_t)out) & 7) return IIR_EINVAL;
    if (ws_bytes < p.ws_bytes || out_bytes < p.out_bytes) return IIR_EINVAL;
    const Geo g = {C, H, W, src_u8 != 0, crop_border, p.hg, p.wg};
    const long plane = (long)p.hg * p.wg;
    float* grey = (float*)ws;
    float* half = grey + (long)N * plane;
    const long nb = (long)p.nbh * p.nbw;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    hipLaunchKernelGGL(niqe_grey_kernel, dim3((unsigned)((plane + NPT - 1) / NPT), (unsigned)N), dim3(NPT), 0, s, src, g, grey);
    hipLaunchKernelGGL(niqe_half_kernel, dim3((unsigned)((plane / 4 + NPT - 1) / NPT), (unsigned)N), dim3(NPT), 0, s, (const float*)grey, p.hg,
                       p.wg, half);
    hipLaunchKernelGGL(niqe_block_kernel<BLK>, dim3(p.nbw, p.nbh, (unsigned)N), dim3(NT), 0, s, (const float*)grey, p.hg, p.wg, out,
                       2 * nb * NSTAT);
    hipLaunchKernelGGL(niqe_block_kernel<BLK / 2>, dim3(p.nbw, p.nbh, (unsigned)N), dim3(NT), 0, s, (const float*)half, p.hg / 2, p.wg / 2,
                       out + nb * NSTAT, 2 * nb * NSTAT);
    return iir_launch_status();
}
