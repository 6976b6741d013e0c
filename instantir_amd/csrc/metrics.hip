// Full-reference image quality on the device: per-image MSE (for PSNR) and SSIM with the definitions restoration papers use
// (no reference counterpart; contract in include/instantir_hip.h: iir_image_metrics, and DESIGN.md section 7 "Image metrics").
// Compiled with -ffp-contract=off like lqfidelity.hip and resample.hip: the tap sums are written with fmaf, so they are fused
// by statement and nothing else is.
//
// The tiled form of lqfidelity.hip.  A workgroup owns a T x T tile of the SSIM map of one image and channel: it stages both
// images for the tile plus the 10-pixel halo of the 11 x 11 window in LDS -- the u8 / fp32 read, the x 255, the quantise and
// the Y conversion happen on the way in, and what is staged is the value minus 128: variances and covariances do not see the
// shift, and E[a^2] - mu^2 loses a quarter of what it loses at 0..255 -- filters the five moments (a, b, a^2, b^2, ab) along x
// into a second LDS image, filters that along y, forms the map and sums its tile.  The squared differences of the pixels the
// tile owns are summed while staging: a pixel belongs to the tile whose T x T square holds it, and the last tile of a row or
// column also owns the 10 pixels past the map's extent, so the MSE covers the whole cropped image.  Every thread's few-term
// fp32 sum goes to fp64, the workgroup adds in a fixed order (wave butterflies, then the four waves in order) and writes its
// two partial sums; a second launch adds each image's partial sums in fp64 (256 strided sequences in index order, then a
// fixed tree) and writes {MSE, SSIM}.  The MSE alone is a launch of its own with no LDS image and no filter arithmetic.
// Every global load is unconditional, from an address clamped into the cropped image; what a clamped
// address gave for a pixel outside the image is replaced by 0 in registers, and only stores are guarded.  No atomics, no
// scratch: equal inputs give equal bits.
#include "image_common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int T = IIR_METRICS_TILE;                 // map tile per axis; 256 threads, each owning T / ROWS map values of one column
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int S = T + HALO;                         // staged rows and columns
constexpr int SP = S + 1;                           // staged row pitch
constexpr int NT = 256, ROWS = NT / T;
constexpr int STAGE = (S * S + NT - 1) / NT;        // staged pixels per thread: 7 squares below 2^16 sum exactly in fp32
constexpr int PE = 8;                               // pixels per thread of the MSE-only launch: 8 such squares do too
constexpr float PIVOT = 128.0f;
constexpr float C1 = 6.5025f, C2 = 58.5225f;        // (0.01 * 255)^2, (0.03 * 255)^2
static_assert(NT % T == 0 && T % ROWS == 0, "a thread keeps its column through both passes");
static_assert((2 * S * SP + 5 * S * T) * sizeof(float) <= 48 * 1024, "static LDS");
static_assert(STAGE * 65025 < (1 << 24) && PE * 65025 < (1 << 24), "a thread's sum of 8-bit squared differences is exact in fp32");

// g_j = exp(-(j - 5)^2 / (2 * 1.5^2)) / sum, formed in fp64 and rounded to fp32
#define IIR_SSIM_TAPS {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f, \
                       0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}

struct Geo {
    int C, H, W;          // the sources as stored
    int crop, hc, wc;     // dropped border; rows and columns that remain
    int y;                // Y of BT.601 instead of the channels
};

// plane `plane` (a channel, or the luma) of pixel (y, x) of image n in 0..255 units
__device__ __forceinline__ float pixel(const ImageSrc& s, const Geo& g, int n, int plane, int y, int x) {
    if (!g.y) return image_load255(s, g.C, g.H, g.W, n, plane, y, x);
    return luma_bt601(image_load255(s, g.C, g.H, g.W, n, 0, y, x), image_load255(s, g.C, g.H, g.W, n, 1, y, x),
                      image_load255(s, g.C, g.H, g.W, n, 2, y, x));
}

// the workgroup's {sum of squared differences, sum of map values} -> ws[2 * slot], ws[2 * slot + 1]
__device__ __forceinline__ void block_partials(float sq, float sm, double (*red)[NT / 64], long slot, double* ws) {
    block_sum_stage(red, sq, sm);
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * slot] = block_sum(red[0]);
        ws[2 * slot + 1] = block_sum(red[1]);
    }
}

// grid (ceil((wc - 10) / T), ceil((hc - 10) / T), N * planes), NT threads
__global__ __launch_bounds__(NT) void metrics_tile_kernel(const ImageSrc A, const ImageSrc B, const Geo g, int planes, int mh, int mw, double* ws) {
    __shared__ float sa[S * SP], sb[S * SP];     // a - 128, b - 128 over [ty0, ty0 + S) x [tx0, tx0 + S) of the cropped image
    __shared__ float sx[5][S * T];               // their five x-filtered moments over the same rows, the tile's columns
    __shared__ double red[2][NT / 64];
    constexpr float taps[WIN] = IIR_SSIM_TAPS;
    const int tid = threadIdx.x, tx = tid % T, tr = tid / T;
    const int tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const int n = blockIdx.z / planes, plane = blockIdx.z - n * planes;

    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < STAGE; ++k) {
        const int i = tid + k * NT, ic = min(i, S * S - 1);
        const int ly = ic / S, lx = ic - ly * S;
        const int gy = ty0 + ly, gx = tx0 + lx;
        const bool inside = i < S * S && gy < g.hc && gx < g.wc;
        const int yy = g.crop + min(gy, g.hc - 1), xx = g.crop + min(gx, g.wc - 1);
        float pa = pixel(A, g, n, plane, yy, xx), pb = pixel(B, g, n, plane, yy, xx);
        pa = inside ? pa : 0.0f;
        pb = inside ? pb : 0.0f;
        if (i < S * S) {
            sa[ly * SP + lx] = pa - PIVOT;
            sb[ly * SP + lx] = pb - PIVOT;
        }
        const bool own = inside && (lx < T || last_x) && (ly < T || last_y);
        const float d = pa - pb;
        sq += own ? d * d : 0.0f;
    }
    __syncthreads();
    // x: a column or row past the image holds -128s and feeds only map positions that are never summed
    for (int ly = tr; ly < S; ly += ROWS) {
        const float* ra = sa + ly * SP + tx;
        const float* rb = sb + ly * SP + tx;
        float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
        for (int j = 0; j < WIN; ++j) {
            const float a = ra[j], b = rb[j];
            m0 = fmaf(taps[j], a, m0);
            m1 = fmaf(taps[j], b, m1);
            m2 = fmaf(taps[j], a * a, m2);
            m3 = fmaf(taps[j], b * b, m3);
            m4 = fmaf(taps[j], a * b, m4);
        }
        const int o = ly * T + tx;
        sx[0][o] = m0; sx[1][o] = m1; sx[2][o] = m2; sx[3][o] = m3; sx[4][o] = m4;
    }
    __syncthreads();
    // y, the map and the thread's share of the tile's sum
    float sm = 0.0f;
    for (int y = tr; y < T; y += ROWS) {
        float m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float* col = sx[q] + y * T + tx;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < WIN; ++j) acc = fmaf(taps[j], col[j * T], acc);
            m[q] = acc;
        }
        const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
        const float mu1 = m[0] + PIVOT, mu2 = m[1] + PIVOT;
        const float num = (2.0f * mu1 * mu2 + C1) * (2.0f * s12 + C2);
        const float den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2);
        const float v = num / den;
        sm += (ty0 + y < mh && tx0 + tx < mw) ? v : 0.0f;
    }
    const long slot = (long)n * planes * gridDim.y * gridDim.x + ((long)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_partials(sq, sm, red, slot, ws);
}

// the MSE alone.  grid (ceil(E / (NT * PE)), N), NT threads; E = planes * hc * wc elements per image, plane-major
__global__ __launch_bounds__(NT) void metrics_mse_kernel(const ImageSrc A, const ImageSrc B, const Geo g, long E, double* ws) {
    __shared__ double red[2][NT / 64];
    const int n = blockIdx.y;
    const long plane_elems = (long)g.hc * g.wc;
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < PE; ++k) {
        const long e = ((long)blockIdx.x * PE + k) * NT + threadIdx.x, ec = min(e, E - 1);
        const int plane = (int)(ec / plane_elems);
        const long r = ec - plane * plane_elems;
        const int y = (int)(r / g.wc), x = (int)(r - (long)y * g.wc);
        const float d = pixel(A, g, n, plane, g.crop + y, g.crop + x) - pixel(B, g, n, plane, g.crop + y, g.crop + x);
        sq += e < E ? d * d : 0.0f;
    }
    block_partials(sq, 0.0f, red, (long)n * gridDim.x + blockIdx.x, ws);
}

// grid (N), NT threads: ws holds `parts` {squares, map values} pairs per image
__global__ __launch_bounds__(NT) void metrics_final_kernel(const double* ws, int parts, double mse_count, double map_count, unsigned what,
                                                           double* out) {
    __shared__ double r[2][NT];
    double sum[2];
    final_sum_f64<NT, 2>(ws + 2 * (long)blockIdx.x * parts, parts, r, sum);
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        out[2 * blockIdx.x] = (what & IIR_METRIC_PSNR) ? sum[0] / mse_count : nan;
        out[2 * blockIdx.x + 1] = (what & IIR_METRIC_SSIM) ? sum[1] / map_count : nan;
    }
}

struct Plan {
    int planes, hc, wc, mh, mw, ntx, nty;
    int64_t elems, parts;             // per image: elements under the MSE, workgroups (= partial-sum pairs)
    bool tiled;
};

// the geometry checks of the contract, shared by both entries; the pointers are the caller's
bool plan(const iir_metrics_desc* d, Plan* p) {
    if (!d) return false;
    if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->H > 32768 || d->W > 32768) return false;
    if (d->C != 1 && d->C != 3) return false;
    if (d->y_channel && d->C != 3) return false;
    if (d->crop_border < 0) return false;
    if (d->what == 0 || (d->what & ~(IIR_METRIC_PSNR | IIR_METRIC_SSIM))) return false;
    const int64_t hc = (int64_t)d->H - 2 * (int64_t)d->crop_border, wc = (int64_t)d->W - 2 * (int64_t)d->crop_border;
    if (hc <= 0 || wc <= 0) return false;
    p->tiled = (d->what & IIR_METRIC_SSIM) != 0;
    if (p->tiled && (hc < WIN || wc < WIN)) return false;
    p->planes = d->y_channel ? 1 : d->C;
    if ((int64_t)d->N * p->planes > 65535) return false;                                      // grid.z / grid.y
    p->hc = (int)hc; p->wc = (int)wc;
    p->elems = (int64_t)p->planes * hc * wc;
    if (p->tiled) {
        p->mh = p->hc - HALO; p->mw = p->wc - HALO;
        p->ntx = (p->mw + T - 1) / T; p->nty = (p->mh + T - 1) / T;
        p->parts = (int64_t)p->planes * p->nty * p->ntx;
    } else {
        p->mh = p->mw = p->ntx = p->nty = 0;
        p->parts = (p->elems + NT * PE - 1) / (NT * PE);
    }
    if (p->parts * d->N > 0x7fffffffLL) return false;
    return true;
}

}  // namespace

extern "C" int64_t iir_image_metrics_workspace_bytes(const iir_metrics_desc* d) {
    Plan p;
    if (!plan(d, &p)) return -1;
    return p.parts * d->N * 2 * (int64_t)sizeof(double);
}

extern "C" int iir_image_metrics(const iir_metrics_desc* d, void* stream) {
    Plan p;
    if (!plan(d, &p)) return IIR_EINVAL;
    if (!d->a || !d->b || !d->out || !d->ws) return IIR_EINVAL;
    if (((uintptr_t)d->ws | (uintptr_t)d->out) & 7) return IIR_EINVAL;
    if (d->ws_bytes < p.parts * d->N * 2 * (int64_t)sizeof(double)) return IIR_EINVAL;
    const ImageSrc A = {d->a, d->a_u8 != 0, d->a_quantize != 0}, B = {d->b, d->b_u8 != 0, d->b_quantize != 0};
    const Geo g = {d->C, d->H, d->W, d->crop_border, p.hc, p.wc, d->y_channel != 0};
    double* ws = (double*)d->ws;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (p.tiled) {
        hipLaunchKernelGGL(metrics_tile_kernel, dim3(p.ntx, p.nty, (unsigned)(d->N * p.planes)), dim3(NT), 0, s, A, B, g, p.planes, p.mh, p.mw, ws);
    } else {
        hipLaunchKernelGGL(metrics_mse_kernel, dim3((unsigned)p.parts, (unsigned)d->N), dim3(NT), 0, s, A, B, g, (long)p.elems, ws);
    }
    hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)d->N), dim3(NT), 0, s, (const double*)ws, (int)p.parts, (double)p.elems,
                       (double)p.planes * p.mh * p.mw, (unsigned)d->what, d->out);
    return iir_launch_status();
}
