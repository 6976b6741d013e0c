// LQ fidelity guidance (no reference counterpart; contract in include/instantir_hip.h: iir_lq_fidelity_f32, and DESIGN.md
// section 7 "LQ fidelity"): after a scheduler step, pull the step's predicted clean latent toward the LQ latent,
//   delta = w * LP(lq - x0),   x0' = x0 + delta,   prev' = prev + c * delta,   hist' = x0'
// LP a separable Gaussian over the latent grid whose out-of-image taps are dropped and whose axes are renormalised by the sum of
// the taps that stayed.  fp32 planar tensors, compiled with -ffp-contract=off like pointwise.hip and regionmap.hip.
//
// A workgroup owns a TX x TY output tile of one plane: it stages d = lq - x0 for the tile and its halo in LDS, filters along x
// into a second LDS image (halo rows included), filters that along y and updates the pixels of its own tile.  Neighbours read
// x0_in through their halos, so x0' goes to a second plane; prev and hist are read and written by the one thread that owns the
// pixel.  Radius 0 (LP = identity) is a launch of its own with no LDS and no filter arithmetic.  The taps are summed in index
// order with fmaf and nothing is atomic: equal inputs give equal bits.
// Every global load is unconditional, from a clamped address; a tap outside the image is masked in
// registers (weight 0 on the finite value the clamped address gave), and only stores are guarded (the one-thread-per-element
// launch of radius 0 ends its surplus threads at entry, as the step kernels of pointwise.hip do).
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int RMAX = IIR_LQ_FIDELITY_MAX_RADIUS;
constexpr int TX = IIR_LQ_FIDELITY_TILE, TY = IIR_LQ_FIDELITY_TILE;    // output tile; 256 threads, each owning TY / ROWS outputs of one column
constexpr int NT = 256, ROWS = NT / TX;
constexpr int SW_MAX = TX + 2 * RMAX, SH_MAX = TY + 2 * RMAX;
static_assert(NT % TX == 0 && TY % ROWS == 0, "a thread keeps its column through both passes");
static_assert((SH_MAX * SW_MAX + SH_MAX * TX) * sizeof(float) <= 64 * 1024, "static LDS");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// 1 for a coordinate inside [0, n), else 0: a tap is masked by this factor (t * 1 and t * 0 are exact), not by a branch
__device__ __forceinline__ float inside01(int v, int n) { return (float)(int)(v >= 0 && v < n); }

// The pointwise half, shared by both kernels: `lp` is LP(lq - x0) at element o; `inside` guards the stores alone.
__device__ __forceinline__ void apply(float lp, long o, bool inside, float w, float c, const float* x0_in, float* prev, float* x0_out,
                                      float* hist) {
    float x0 = x0_in[o];
    float pv = prev[o];
    asm volatile("" : "+v"(x0), "+v"(pv));      // opaque here: keeps hipcc from sinking the two loads under the store guard
    const float delta = w * lp;
    const float x0n = x0 + delta;
    if (inside) {
        x0_out[o] = x0n;
        prev[o] = pv + c * delta;
        if (hist) hist[o] = x0n;
    }
}

// radius 0: one thread per element
__global__ __launch_bounds__(NT) void lq_fidelity_point_kernel(const float* x0_in, const float* lq, const float* wc, long n, float* prev,
                                                               float* x0_out, float* hist) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    apply(lq[i] - x0_in[i], i, true, wc[0], wc[1], x0_in, prev, x0_out, hist);
}

// grid (ceil(W / TX), ceil(H / TY), planes), NT threads; 1 <= r <= RMAX, taps[2r + 1]
__global__ __launch_bounds__(NT) void lq_fidelity_tile_kernel(const float* x0_in, const float* lq, const float* __restrict__ taps, int r,
                                                              const float* wc, int H, int W, float* prev, float* x0_out,
                                                              float* hist) {
    __shared__ float sd[SH_MAX * SW_MAX];        // d = lq - x0 over [ty0 - r, ty0 + TY + r) x [tx0 - r, tx0 + TX + r), clamped
    __shared__ float sx[SH_MAX * TX];            // its x-filtered form over the same rows, the tile's columns
    const int tid = threadIdx.x, tx = tid % TX, tr = tid / TX;
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int SW = TX + 2 * r, SH = TY + 2 * r, k = 2 * r + 1;
    const long base = (long)blockIdx.z * H * W;
    const float w = wc[0], c = wc[1];

    for (int i = tid; i < SH * SW; i += NT) {
        const int ly = i / SW, lx = i - ly * SW;
        const long o = base + (long)clampi(ty0 - r + ly, 0, H - 1) * W + clampi(tx0 - r + lx, 0, W - 1);
        sd[i] = lq[o] - x0_in[o];
    }
    __syncthreads();
    // x: a column past the image has no tap inside it (norm 0) and is never read by the y pass of a stored pixel
    for (int ly = tr; ly < SH; ly += ROWS) {
        const float* row = sd + ly * SW + tx;
        float acc = 0.0f, norm = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int gx = tx0 + tx + j - r;
            const float t = taps[j] * inside01(gx, W);
            acc = fmaf(t, row[j], acc);
            norm += t;
        }
        sx[ly * TX + tx] = norm > 0.0f ? acc / norm : 0.0f;
    }
    __syncthreads();
    // y, and the update of the tile's own pixels
    for (int y = tr; y < TY; y += ROWS) {
        const float* col = sx + y * TX + tx;
        float acc = 0.0f, norm = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int gy = ty0 + y + j - r;
            const float t = taps[j] * inside01(gy, H);
            acc = fmaf(t, col[j * TX], acc);
            norm += t;
        }
        const int gx = tx0 + tx, gy = ty0 + y;
        const bool inside = gx < W && gy < H;
        const long o = base + (long)min(gy, H - 1) * W + min(gx, W - 1);
        apply(norm > 0.0f ? acc / norm : 0.0f, o, inside, w, c, x0_in, prev, x0_out, hist);
    }
}

}  // namespace

extern "C" int iir_lq_fidelity_f32(const float* x0_in, const float* lq, const float* taps, int32_t radius, const float* wc, int32_t planes,
                                   int32_t H, int32_t W, float* prev, float* x0_out, float* hist, void* stream) {
    if (!x0_in || !lq || !wc || !prev || !x0_out) return IIR_EINVAL;
    if (radius < 0 || radius > RMAX || (radius > 0 && !taps)) return IIR_EINVAL;
    if (planes <= 0 || planes > 65535 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return IIR_EINVAL;
    // neighbours read x0_in (and lq) through their halos: no output may be one of them; each output is a plane of its own
    if (x0_out == x0_in || x0_out == lq || prev == x0_in || prev == lq || prev == x0_out) return IIR_EINVAL;
    if (hist && (hist == x0_in || hist == lq || hist == prev || hist == x0_out)) return IIR_EINVAL;
    const long n = (long)planes * H * W;
    if ((n + NT - 1) / NT > 0x7fffffffL) return IIR_EINVAL;
    (void)hipGetLastError();
    if (radius == 0) {
        hipLaunchKernelGGL(lq_fidelity_point_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, x0_in, lq, wc, n,
                           prev, x0_out, hist);
    } else {
        hipLaunchKernelGGL(lq_fidelity_tile_kernel, dim3((W + TX - 1) / TX, (H + TY - 1) / TY, (unsigned)planes), dim3(NT), 0,
                           (hipStream_t)stream, x0_in, lq, taps, (int)radius, wc, (int)H, (int)W, prev, x0_out, hist);
    }
    return iir_launch_status();
}
