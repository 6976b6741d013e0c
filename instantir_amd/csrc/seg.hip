// Smoothed-energy guidance (SEG; Hong 2024, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of
// Attention"): the separable Gaussian blur of the queries of the perturbed batch rows over the token grid, in place in the
// q | k buffer the fused projection wrote (include/instantir_hip.h: iir_seg_blur_q_f16).
//
// One workgroup owns one (image, channel chunk) slab of H x W tokens: it reads the slab, filters along x into an fp32 copy in
// LDS, filters that along y and stores fp16 over the slab it read.  No other workgroup touches those bytes, and every read of
// global memory is behind a barrier before the first store, so the update in place is safe by construction.  The chunk is 8
// channels (16-byte accesses) while the fp32 slab fits LDS -- up to 64 x 64 tokens, every SDXL level up to 1024^2 -- and 2
// channels for grids up to 128 x 128.  The taps are summed in index order with fmaf, the tree of the mean mode has a fixed
// shape, and nothing is atomic: equal inputs give equal bits.
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int NT = 1024;                   // 16 waves: one workgroup per CU at the SDXL sizes, so the waves hide the LDS latency
constexpr int STAGE_TOK = 1024;            // tokens of fp16 input staged per x-pass batch (whole rows; one row when W is larger)
constexpr int MAX_EXTENT = IIR_SEG_MAX_EXTENT;
constexpr int WIDE_TOKENS = 4096;          // the 8-channel chunk: 4096 x 8 fp32 = 128 KiB of the CU's 160

template <int CW> struct Chunk;
template <> struct Chunk<8> { using V = f16x8; };
template <> struct Chunk<2> { using V = f16x2; };

__host__ __device__ inline int stage_rows(int W) { return STAGE_TOK / W > 0 ? STAGE_TOK / W : 1; }

// `n - 1 + i` -> `n - 1 - i`, `-i` -> `i`; |offset| <= n - 1, so one fold lands inside
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// grid (C / CW, images), NT threads, dynamic LDS: float[T][CW] | V[stage_rows(W) * W]
template <int CW>
__global__ __launch_bounds__(NT) void seg_blur_kernel(f16* q, long ldq, int H, int W, const float* __restrict__ wy, int ky,
                                                       const float* __restrict__ wx, int kx, int mean) {
    using V = typename Chunk<CW>::V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = H * W, tid = threadIdx.x;
    float* inter = (float*)smem;
    V* stage = (V*)(smem + (size_t)T * CW * sizeof(float));
    f16* base = q + (long)blockIdx.y * T * ldq + (long)blockIdx.x * CW;

    if (mean) {
        // sigma beyond the cut-off: every token becomes its image's mean.  Pairwise tree over the tokens, ceil(log2 T) levels.
        for (int t = tid; t < T; t += NT) {
            const V v = *(const V*)(base + (long)t * ldq);
#pragma unroll
            for (int c = 0; c < CW; ++c) inter[t * CW + c] = (float)v[c];
        }
        __syncthreads();
        int P = 1;
        while (P < T) P <<= 1;
        for (int s = P >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < s; t += NT)
                if (t + s < T) {
#pragma unroll
                    for (int c = 0; c < CW; ++c) inter[t * CW + c] += inter[(t + s) * CW + c];
                }
            __syncthreads();
        }
        V o;
#pragma unroll
        for (int c = 0; c < CW; ++c) o[c] = (f16)(inter[c] / (float)T);
        for (int t = tid; t < T; t += NT) *(V*)(base + (long)t * ldq) = o;
        return;
    }

    // x: fp16 rows staged in LDS -> fp32 slab
    const int rx = kx >> 1, ry = ky >> 1;
    const int rows_per = stage_rows(W);
    for (int y0 = 0; y0 < H; y0 += rows_per) {
        const int n = min(rows_per, H - y0) * W;
        for (int i = tid; i < n; i += NT) stage[i] = *(const V*)(base + (long)(y0 * W + i) * ldq);
        __syncthreads();
        for (int i = tid; i < n; i += NT) {
            const int yl = i / W, x = i - yl * W;
            const V* row = stage + yl * W;
            float acc[CW];
#pragma unroll
            for (int c = 0; c < CW; ++c) acc[c] = 0.0f;
#pragma unroll 4
            for (int j = 0; j < kx; ++j) {
                const V v = row[reflect(x + j - rx, W)];
                const float w = wx[j];
#pragma unroll
                for (int c = 0; c < CW; ++c) acc[c] = fmaf(w, (float)v[c], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) inter[(y0 * W + i) * CW + c] = acc[c];
        }
        __syncthreads();
    }
    // y: fp32 slab -> fp16 over the tokens this workgroup read
    for (int t = tid; t < T; t += NT) {
        const int y = t / W, x = t - y * W;
        float acc[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) acc[c] = 0.0f;
#pragma unroll 4
        for (int j = 0; j < ky; ++j) {
            const float* p = inter + (reflect(y + j - ry, H) * W + x) * CW;
            const float w = wy[j];
#pragma unroll
            for (int c = 0; c < CW; ++c) acc[c] = fmaf(w, p[c], acc[c]);
        }
        V o;
#pragma unroll
        for (int c = 0; c < CW; ++c) o[c] = (f16)acc[c];
        *(V*)(base + (long)t * ldq) = o;
    }
}

template <int CW>
int launch(f16* q, long ldq, int images, int H, int W, int C, const float* wy, int ky, const float* wx, int kx, int mean,
           hipStream_t stream) {
    const size_t lds = (size_t)H * W * CW * sizeof(float) + (size_t)stage_rows(W) * W * CW * sizeof(f16);
    constexpr size_t lds_max = (size_t)(CW == 8 ? WIDE_TOKENS : MAX_EXTENT * MAX_EXTENT) * CW * sizeof(float)
                               + (size_t)STAGE_TOK * CW * sizeof(f16);
    static unsigned long long lds_set = 0;
    if (!iir_ensure_dynamic_lds((const void*)seg_blur_kernel<CW>, lds_max, lds_set)) return IIR_ELAUNCH;
    hipLaunchKernelGGL(seg_blur_kernel<CW>, dim3(C / CW, images), dim3(NT), lds, stream, q, ldq, H, W, wy, ky, wx, kx, mean);
    return iir_launch_status();
}

bool taps_ok(const float* w, int k, int n) { return w && k >= 1 && (k & 1) && k / 2 <= n - 1; }

}  // namespace

extern "C" int iir_seg_blur_q_f16(void* q, int64_t ldq, int32_t images, int32_t H, int32_t W, int32_t C, const float* wy, int32_t ky,
                                  const float* wx, int32_t kx, int32_t mean, void* stream) {
    if (!q || ((uintptr_t)q & 15) || images <= 0 || images > 65535 || H <= 0 || W <= 0 || C <= 0 || C % 8) return IIR_EINVAL;
    if (H > MAX_EXTENT || W > MAX_EXTENT || ldq < C || ldq % 8) return IIR_EINVAL;
    if (!mean && (!taps_ok(wy, ky, H) || !taps_ok(wx, kx, W))) return IIR_EINVAL;
    (void)hipGetLastError();
    if (H * W <= WIDE_TOKENS)
        return launch<8>((f16*)q, (long)ldq, images, H, W, C, wy, ky, wx, kx, mean ? 1 : 0, (hipStream_t)stream);
    return launch<2>((f16*)q, (long)ldq, images, H, W, C, wy, ky, wx, kx, mean ? 1 : 0, (hipStream_t)stream);
}
