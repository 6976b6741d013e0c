// What the image kernels (metrics.hip, niqe.hip, lpips.hip, dists.hip, resample.hip) agree on, defined once: which pixel a source
// holds, the rounding to the 8-bit grid, the BT.601 luma, the 16-bit channel access and ReLU of the two VGG-16 scorers, and the
// fixed summation orders that make equal inputs give equal bits.  Included by those five files only; each is compiled with -ffp-contract=off, so nothing here is fused that is not written as
// fmaf, and every statement below keeps its operands and their order.
#pragma once
#include "common.h"

// to the 8-bit grid: the value an 8-bit image file would hold
__device__ __forceinline__ float round_u8(float v) { return fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f); }

// An image batch as uploaded: uint8 interleaved (N, H, W, C), or fp32 planar (N, C, H, W) on a [0, 1] scale, which `quantize`
// rounds to the 8-bit grid on the way in (a uint8 source is on it).
struct ImageSrc {
    const void* p;
    int u8, quantize;
};

// channel `ch` of pixel (y, x) of image n in 0..255 units; (y, x) in source coordinates, inside the image
__device__ __forceinline__ float image_load255(const ImageSrc& s, int C, int H, int W, int n, int ch, int y, int x) {
    if (s.u8) return (float)((const uint8_t*)s.p)[(((long)n * H + y) * W + x) * C + ch];
    float v = ((const float*)s.p)[(((long)n * C + ch) * H + y) * W + x] * 255.0f;
    if (s.quantize) v = round_u8(v);
    return v;
}

// Y of BT.601 (16..235) from R, G, B in 0..255 units
__device__ __forceinline__ float luma_bt601(float r, float g, float b) {
    float t = 65.481f * r;
    t = t + 128.553f * g;
    t = t + 24.966f * b;
    return 16.0f + t / 255.0f;
}

// eight consecutive 16-bit channels (fp16 or bf16, 16-byte aligned) as one load or store, held in fp32 (lpips.hip, dists.hip)
template <typename E> __device__ __forceinline__ void load8(const E* p, float (&v)[8]) {
    const typename ET<E>::x8 r = *(const typename ET<E>::x8*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
}

template <typename E> __device__ __forceinline__ void store8(E* p, const float (&v)[8]) {
    typename ET<E>::x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (E)v[i];
    *(typename ET<E>::x8*)p = r;
}

// NaN stays NaN (a comparison with it is false), so an overflow upstream still shows in the distance and in the sums
__device__ __forceinline__ float relu_f(float x) { return x < 0.0f ? 0.0f : x; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The workgroup's sums of one or more values per thread in a fixed order, in two steps around the caller's __syncthreads(): every
// thread calls block_sum_stage (value k goes to fp64 and through the wave butterflies, then lane 0 of wave w leaves its wave's
// sums in red[k][w]), then any thread may call block_sum (the NW waves of one row of red in index order).
template <int NW, typename... T> __device__ __forceinline__ void block_sum_stage(double (*red)[NW], T... v) {
    const double s[] = {wave_sum_f64((double)v)...};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < (int)sizeof...(T); ++k) red[k][threadIdx.x >> 6] = s[k];
    }
}

template <int NW> __device__ __forceinline__ double block_sum(const double (&red)[NW]) {
    double a = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) a += red[w];
    return a;
}

// The second stage: a workgroup of NT threads adds `parts` rows of COLS interleaved partial sums at p, column by column.  Thread
// t adds rows t, t + NT, ... in index order, then a halving tree in LDS; out[c] is column c's sum, valid in thread 0.
template <int NT, int COLS> __device__ __forceinline__ void final_sum_f64(const double* p, int parts, double (*r)[NT], double (&out)[COLS]) {
    const int tid = threadIdx.x;
    double q[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) q[c] = 0.0;
    for (int i = tid; i < parts; i += NT) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) q[c] += p[COLS * i + c];
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) r[c][tid] = q[c];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int c = 0; c < COLS; ++c) r[c][tid] += r[c][tid + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) out[c] = r[c][0];
}

// whether the byte ranges [p, p + pbytes) and [q, q + qbytes) meet
static inline bool overlap(const void* p, int64_t pbytes, const void* q, int64_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}
