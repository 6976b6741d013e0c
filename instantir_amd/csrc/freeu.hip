// FreeU on the decoder's skip concat (module/min_sdxl.py:22-77 `fourier_filter` / `apply_freeu`, applied before the
// torch.cat of CrossAttnUpBlock2D / UpBlock2D, module/unet/unet_2d_ZeroSFT_blocks.py:2600-2627,2748-2775).
// Compiled with -ffp-contract=off: `skip + add * scale` is formed exactly as copy_add_kernel (pointwise.hip) forms it, so
// with s = 1, b = 1 the concat is bit-identical to the two copy_add launches it replaces.
//
// The filter (threshold 1) scales the fftshift-ed centre [H/2-1, H/2+1) x [W/2-1, W/2+1) of the 2-D spectrum by s, i.e. the
// DFT frequencies {0, -1 mod H} x {0, -1 mod W} (duplicates dropped when H or W is 1).  Per (image, channel) plane v:
//   y[h,w] = v[h,w] + (s - 1) / (H W) * sum_{(a,b) in F} (C_ab cos phi_ab(h,w) + S_ab sin phi_ab(h,w))
//   phi_ab = 2 pi (a h / H + b w / W),  C_ab = sum v cos phi_ab,  S_ab = sum v sin phi_ab,  F = {(0,0),(1,0),(0,1),(1,1)}
// (the real part is even in the frequency pair, so -1 becomes +1 in both axes: the diagonal (1,1)).  Seven fp32 sums per
// plane: freeu_stats_kernel leaves them per HW slab, freeu_concat_kernel merges the slabs in a fixed order and writes
// cat = [x (+ mid residual), first half of its channels times b | filter_s(skip (+ residual))].
//
// No float atomics, no cross-lane exchange: loads are unconditional from clamped addresses, invalid rows are
// selected out, and the reductions go through LDS in a fixed order.
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int NSLAB = IIR_FREEU_SLABS;   // HW slabs per (image, channel): partials[R][NSLAB][7][C]
constexpr int NSUM = 7;                  // sum v | C10 S10 | C01 S01 | C11 S11
constexpr int CB = 64;                   // channels per workgroup: 8 lanes x 8 halves
constexpr int RL = 32;                   // row lanes per workgroup (256 threads)
constexpr int CONCAT_ROWS = 256;         // rows of one image per concat workgroup (8 per thread)

// sin / cos of pi * 2n/N, argument reduced to (-1, 1] from the exact integer phase (never an accumulated angle)
__device__ __forceinline__ void phase_sc(int n, int N, float* s, float* c) {
    int m = 2 * n;
    if (m > N) m -= 2 * N;
    sincospif((float)m / (float)N, s, c);
}

// the three (sin, cos) pairs of pixel p = h * W + w: phi10, phi01, phi11
__device__ __forceinline__ void pixel_trig(int p, int H, int W, float sc[6]) {
    const int h = p / W, w = p - h * W;
    const int HW = H * W;
    int n11 = h * W + w * H;
    if (n11 >= HW) n11 -= HW;
    phase_sc(h, H, &sc[1], &sc[0]);
    phase_sc(w, W, &sc[3], &sc[2]);
    phase_sc(n11, HW, &sc[5], &sc[4]);
}

// grid (R * NSLAB, ceil(C / 64)), 256 threads
__global__ __launch_bounds__(256) void freeu_stats_kernel(const f16* sk, long lds_, const f16* add, long lda, const float* add_scale,
                                                           int H, int W, int C, float* part) {
    __shared__ float red[RL][NSUM][CB];
    const int tid = threadIdx.x, oct = tid & 7, rl = tid >> 3;
    const int r = blockIdx.x / NSLAB, slab = blockIdx.x % NSLAB;
    const int HW = H * W;
    const int per = (HW + NSLAB - 1) / NSLAB;
    const int lo = min(slab * per, HW), hi = min(lo + per, HW);
    const int c0 = blockIdx.y * CB + oct * 8;
    const int cl = min(c0, C - 8);                                   // clamped channel octet: loads stay in bounds
    const float sc_r = add_scale ? add_scale[r] : 1.0f;
    float acc[NSUM][8];
#pragma unroll
    for (int k = 0; k < NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.0f;
    const int iters = (per + RL - 1) / RL;
    for (int it = 0; it < iters; ++it) {
        const int p = lo + it * RL + rl;
        const bool valid = p < hi;
        const int pl = min(p, HW - 1);
        const long m = (long)r * HW + pl;
        f16x8 v = *(const f16x8*)(sk + m * lds_ + cl);
        float t[8];
        if (add) {
            const f16x8 a = *(const f16x8*)(add + m * lda + cl);
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (float)v[j] + (float)a[j] * sc_r;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (float)v[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = valid ? t[j] : 0.0f;
        float tr[6];
        pixel_trig(pl, H, W, tr);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[0][j] += t[j];
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[1 + k][j] += t[j] * tr[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[rl][k][oct * 8 + j] = acc[k][j];
    __syncthreads();
    for (int idx = tid; idx < NSUM * CB; idx += 256) {
        const int k = idx / CB, c = idx % CB;
        float s = 0.0f;
        for (int q = 0; q < RL; ++q) s += red[q][k][c];
        const int cg = blockIdx.y * CB + c;
        if (cg < C) part[(((long)r * NSLAB + slab) * NSUM + k) * C + cg] = s;
    }
}

// grid (R * ceil(HW / 256), ceil(cx / 64) + ceil(cs / 64)), 256 threads.  Column blocks below ceil(cx / 64) write the
// hidden half, the others the filtered skip.
__global__ __launch_bounds__(256) void freeu_concat_kernel(const f16* x, long ldx, int cx, const f16* mid, long ldm, const f16* sk,
                                                            long lds_, int cs, const f16* add, long lda, const float* add_scale,
                                                            int H, int W, float b, float s, const float* part, f16* cat,
                                                            long ldc, long cat_off) {
    __shared__ float coef[NSUM][CB];
    const int tid = threadIdx.x, oct = tid & 7, rl = tid >> 3;
    const int HW = H * W;
    const int ntile = (HW + CONCAT_ROWS - 1) / CONCAT_ROWS;
    const int r = blockIdx.x / ntile, p0 = (blockIdx.x % ntile) * CONCAT_ROWS;
    const int nbx = (cx + CB - 1) / CB;
    const float sc_r = add_scale ? add_scale[r] : 1.0f;
    if ((int)blockIdx.y < nbx) {
        // hidden: (x + mid * scale), channels < cx / 2 times b
        const int c0 = blockIdx.y * CB + oct * 8;
        const int cl = min(c0, cx - 8);
        const int half = cx / 2;
#pragma unroll 4
        for (int i = 0; i < CONCAT_ROWS / RL; ++i) {
            const int p = p0 + i * RL + rl;
            const long m = (long)r * HW + min(p, HW - 1);
            const f16x8 v = *(const f16x8*)(x + m * ldx + cl);
            float t[8];
            if (mid) {
                const f16x8 a = *(const f16x8*)(mid + m * ldm + cl);
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = (float)v[j] + (float)a[j] * sc_r;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = (float)v[j];
            }
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (f16)(cl + j < half ? t[j] * b : t[j]);
            if (p < HW && c0 < cx) *(f16x8*)(cat + m * ldc + cat_off + c0) = o;
        }
        return;
    }
    // skip: merge the slab partials of this workgroup's 64 channels (slab order fixed), drop duplicate frequencies
    const int cb = blockIdx.y - nbx;
    for (int idx = tid; idx < NSUM * CB; idx += 256) {
        const int k = idx / CB, c = idx % CB;
        const int cc = min(cb * CB + c, cs - 1);
        float a = 0.0f;
        for (int sl = 0; sl < NSLAB; ++sl) a += part[(((long)r * NSLAB + sl) * NSUM + k) * cs + cc];
        const bool keep = k == 0 || ((k == 1 || k == 2) && H > 1) || ((k == 3 || k == 4) && W > 1) || (k >= 5 && H > 1 && W > 1);
        coef[k][c] = keep ? a : 0.0f;
    }
    __syncthreads();
    const int c0 = cb * CB + oct * 8;
    const int cl = min(c0, cs - 8);
    float cf[NSUM][8];
#pragma unroll
    for (int k = 0; k < NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) cf[k][j] = coef[k][oct * 8 + j];
    const float ks = (s - 1.0f) / (float)HW;
#pragma unroll 4
    for (int i = 0; i < CONCAT_ROWS / RL; ++i) {
        const int p = p0 + i * RL + rl;
        const int pl = min(p, HW - 1);
        const long m = (long)r * HW + pl;
        const f16x8 v = *(const f16x8*)(sk + m * lds_ + cl);
        float t[8];
        if (add) {
            const f16x8 a = *(const f16x8*)(add + m * lda + cl);
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (float)v[j] + (float)a[j] * sc_r;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (float)v[j];
        }
        if (ks != 0.0f) {                                            // s == 1: the copy, bit for bit
            float tr[6];
            pixel_trig(pl, H, W, tr);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float corr = cf[0][j];
#pragma unroll
                for (int k = 0; k < 6; ++k) corr = corr + cf[1 + k][j] * tr[k];
                t[j] = t[j] + ks * corr;
            }
        }
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)t[j];
        if (p < HW && c0 < cs) *(f16x8*)(cat + m * ldc + cat_off + cx + c0) = o;
    }
}

// common checks of a (rows, H, W) plane set; returns R or -1
long planes(int64_t rows, int32_t H, int32_t W) {
    if (rows <= 0 || H < 1 || W < 1 || H > 65535 || W > 65535) return -1;
    const int64_t HW = (int64_t)H * W;
    if (HW > (1 << 26) || rows % HW) return -1;
    const int64_t R = rows / HW;
    if (R > 65535) return -1;
    return (long)R;
}

}  // namespace

extern "C" int64_t iir_freeu_partials_bytes(int64_t rows, int32_t H, int32_t W, int32_t C) {
    const long R = planes(rows, H, W);
    if (R < 0 || C <= 0 || C % 8) return -1;
    return (int64_t)R * NSLAB * NSUM * C * (int64_t)sizeof(float);
}

extern "C" int iir_freeu_stats_f16(const void* skip, int64_t lds, const void* add, int64_t lda, const float* add_scale, int64_t rows,
                                   int32_t H, int32_t W, int32_t C, float* partials, int64_t partials_bytes, void* stream) {
    (void)hipGetLastError();
    const long R = planes(rows, H, W);
    if (!skip || !partials || R < 0 || C <= 0 || C % 8 || lds % 8 || lds < C) return IIR_EINVAL;
    if (add && (lda % 8 || lda < C)) return IIR_EINVAL;
    if (partials_bytes < iir_freeu_partials_bytes(rows, H, W, C)) return IIR_EINVAL;
    hipLaunchKernelGGL(freeu_stats_kernel, dim3((unsigned)(R * NSLAB), (C + CB - 1) / CB), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)skip, (long)lds, (const f16*)add, (long)lda, add_scale, H, W, C, partials);
    return iir_launch_status();
}

extern "C" int iir_freeu_concat_f16(const void* x, int64_t ldx, int32_t cx, const void* mid_add, int64_t ldm, const void* skip,
                                    int64_t lds, int32_t cs, const void* add, int64_t lda, const float* add_scale, int64_t rows,
                                    int32_t H, int32_t W, float b, float s, const float* partials, int64_t partials_bytes,
                                    void* cat, int64_t ldc, int64_t cat_off, void* stream) {
    (void)hipGetLastError();
    const long R = planes(rows, H, W);
    if (!x || !skip || !cat || !partials || R < 0) return IIR_EINVAL;
    if (cx <= 0 || cx % 8 || cs <= 0 || cs % 8 || ldx % 8 || ldx < cx || lds % 8 || lds < cs) return IIR_EINVAL;
    if (mid_add && (ldm % 8 || ldm < cx)) return IIR_EINVAL;
    if (add && (lda % 8 || lda < cs)) return IIR_EINVAL;
    if (ldc % 8 || cat_off < 0 || cat_off % 8 || ldc < cat_off + cx + cs) return IIR_EINVAL;
    if (partials_bytes < iir_freeu_partials_bytes(rows, H, W, cs)) return IIR_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const int ntile = (int)((HW + CONCAT_ROWS - 1) / CONCAT_ROWS);
    hipLaunchKernelGGL(freeu_concat_kernel, dim3((unsigned)(R * ntile), (cx + CB - 1) / CB + (cs + CB - 1) / CB), dim3(256), 0,
                       (hipStream_t)stream, (const f16*)x, (long)ldx, cx, (const f16*)mid_add, (long)ldm, (const f16*)skip, (long)lds,
                       cs, (const f16*)add, (long)lda, add_scale, H, W, b, s, partials, (f16*)cat, (long)ldc, (long)cat_off);
    return iir_launch_status();
}
