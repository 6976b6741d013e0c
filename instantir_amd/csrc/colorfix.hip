// LQ-guided colour correction of the decoded image (no reference counterpart; the definitions are StableSR's
// `wavelet_color_fix` / `adain_color_fix`, stated in include/instantir_hip.h and DESIGN.md section 7 "Colour fix").
// fp32 planar (B, C, H, W) in, fp32 out, any H, W >= 1.  Compiled with -ffp-contract=off like pointwise.hip.
//
// wavelet: result = clamp(content + Bl(style - content)), Bl = blur_16 . blur_8 . blur_4 . blur_2 . blur_1, each blur_r the
// 3x3 kernel [1,2,1]/4 (x) [1,2,1]/4 at dilation r over a replicate-padded plane.  Replicate padding is an index clamp per
// axis, so the five horizontal 3-tap levels (wavelet_rows_kernel) commute with the five vertical ones (wavelet_cols_kernel);
// every weight is a power of two, so a level rounds twice per element: (a/4 + c/4) + b/2.
// A workgroup holds pixels [lo, hi] of its row (column strip) in LDS: its own outputs plus up to 31 = 1+2+4+8+16 neighbours
// on either side, cut at the image border.  A level reads index clamp(g -+ r, 0, n-1) of the IMAGE; for every element an
// output depends on, that index lies inside [lo, hi] (the dependency cone shrinks by r per level), so the per-level clamp of
// the definition is reproduced exactly and no edge extension is ever formed.
//
// adain: per (image, channel) mean and unbiased std of both inputs.  adain_stats_kernel leaves (n, mean, M2) per HW slab,
// two passes inside the slab (sum, then centred squares); adain_apply_kernel merges the slabs in slab order (in double:
// mean = sum n_i m_i / N, M2 = sum (M2_i + n_i (m_i - mean)^2)) and applies ((x - mean_c) / std_c) * std_s + mean_s.
// No atomics: equal inputs give equal bits.
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int HALO = 31;                     // 1 + 2 + 4 + 8 + 16
constexpr int SEG = 2048;                    // row pass: outputs of one row per workgroup
constexpr int SEGBUF = SEG + 2 * HALO + 2;
constexpr int TW = 32, TH = 128;             // column pass: output tile (columns x rows); 47.5 KiB of LDS, 3 workgroups per CU
constexpr int TROWS = TH + 2 * HALO;
constexpr int NSLAB = IIR_COLORFIX_SLABS;    // HW slabs per plane: partials[2][P][NSLAB][3]
constexpr int APPLY_ELEMS = 4096;            // elements of one plane per adain_apply workgroup
static_assert(NSLAB == 64, "adain_apply_kernel gives each slab of a plane one lane of a wave");

__device__ __forceinline__ float tap3(float a, float b, float c) { return (0.25f * a + 0.25f * c) + 0.5f * b; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// grid (P * H, ceil(W / SEG)), 256 threads.  vec: W % 4 == 0, W <= SEG and 16-byte aligned bases (whole rows, float4).
__global__ __launch_bounds__(256) void wavelet_rows_kernel(const float* content, const float* style, float* d, int W, int vec) {
    __shared__ __attribute__((aligned(16))) float buf[2][SEGBUF];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * W;
    const int s0 = blockIdx.y * SEG, s1 = min(s0 + SEG, W);
    const int lo = max(s0 - HALO, 0), hi = min(s1 + HALO, W) - 1;
    const int n = hi - lo + 1;
    const float* c = content + row;
    const float* s = style + row;
    if (vec) {
        for (int q = tid; q < n / 4; q += 256) *(f32x4*)&buf[0][4 * q] = ((const f32x4*)s)[q] - ((const f32x4*)c)[q];
    } else {
        for (int i = tid; i < n; i += 256) buf[0][i] = s[lo + i] - c[lo + i];
    }
    __syncthreads();
    int cur = 0, rem = HALO;
    for (int r = 1; r <= 16; r <<= 1) {
        rem -= r;                                                    // neighbours still needed after this level
        const int a = max(s0 - rem, lo), b = min(s1 - 1 + rem, hi);
        for (int g = a + tid; g <= b; g += 256)
            buf[cur ^ 1][g - lo] = tap3(buf[cur][clampi(g - r, 0, W - 1) - lo], buf[cur][g - lo], buf[cur][clampi(g + r, 0, W - 1) - lo]);
        __syncthreads();
        cur ^= 1;
    }
    float* o = d + row;
    if (vec) {
        for (int q = tid; q < n / 4; q += 256) ((f32x4*)o)[q] = *(const f32x4*)&buf[cur][4 * q];
    } else {
        for (int g = s0 + tid; g < s1; g += 256) o[g] = buf[cur][g - lo];
    }
}

// grid (ceil(W / TW), ceil(H / TH), P), 256 threads.  vec: W % 4 == 0 and 16-byte aligned bases.
__global__ __launch_bounds__(256) void wavelet_cols_kernel(const float* content, const float* d, float* out, int H, int W, int vec) {
    __shared__ __attribute__((aligned(16))) float buf[2][TROWS][TW];
    const int tid = threadIdx.x;
    const long plane = (long)blockIdx.z * H * W;
    const int w0 = blockIdx.x * TW, h0 = blockIdx.y * TH, h1 = min(h0 + TH, H);
    const int lo = max(h0 - HALO, 0), hi = min(h1 + HALO, H) - 1;
    const int n = hi - lo + 1;
    const int q4 = (tid & 7) * 4, rv = tid >> 3;                     // float4 mapping: 8 quads x 32 rows
    const int cc = tid & 31, rr = tid >> 5;                          // scalar mapping: 32 columns x 8 rows
    // columns at or beyond W are never loaded: a column only feeds itself, and it is never stored
    if (vec) {
        if (w0 + q4 < W)
            for (int j = rv; j < n; j += 32) *(f32x4*)&buf[0][j][q4] = *(const f32x4*)(d + plane + (long)(lo + j) * W + w0 + q4);
    } else {
        if (w0 + cc < W)
            for (int j = rr; j < n; j += 8) buf[0][j][cc] = d[plane + (long)(lo + j) * W + w0 + cc];
    }
    __syncthreads();
    int cur = 0, rem = HALO;
    for (int r = 1; r <= 16; r <<= 1) {
        rem -= r;
        const int a = max(h0 - rem, lo), b = min(h1 - 1 + rem, hi);
        for (int g = a + rr; g <= b; g += 8)
            buf[cur ^ 1][g - lo][cc] = tap3(buf[cur][clampi(g - r, 0, H - 1) - lo][cc], buf[cur][g - lo][cc], buf[cur][clampi(g + r, 0, H - 1) - lo][cc]);
        __syncthreads();
        cur ^= 1;
    }
    if (vec) {
        if (w0 + q4 < W)
            for (int g = h0 + rv; g < h1; g += 32) {
                const long m = plane + (long)g * W + w0 + q4;
                const f32x4 v = *(const f32x4*)(content + m) + *(const f32x4*)&buf[cur][g - lo][q4];
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = clamp01(v[j]);
                *(f32x4*)(out + m) = o;
            }
    } else {
        if (w0 + cc < W)
            for (int g = h0 + rr; g < h1; g += 8) {
                const long m = plane + (long)g * W + w0 + cc;
                out[m] = clamp01(content[m] + buf[cur][g - lo][cc]);
            }
    }
}

// sum over the workgroup in a fixed order (tree over LDS); every thread returns the total
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const float t = red[0];
    __syncthreads();
    return t;
}

// elements of one slab: a multiple of 4, so that slabs of a plane with HW % 4 == 0 start 16-byte aligned
__host__ __device__ __forceinline__ int slab_elems(int HW) { return (((HW + NSLAB - 1) / NSLAB) + 3) & ~3; }

// grid (NSLAB, 2 * P), 256 threads: planes [0, P) of content, then of style.  vec: HW % 4 == 0 and 16-byte aligned bases.
__global__ __launch_bounds__(256) void adain_stats_kernel(const float* content, const float* style, int HW, int P, float* part, int vec) {
    __shared__ float red[256];
    const int tid = threadIdx.x, y = blockIdx.y, slab = blockIdx.x;
    const int per = slab_elems(HW);
    const int lo = min(slab * per, HW), hi = min(lo + per, HW), n = hi - lo;
    const float* x = (y < P ? content + (long)y * HW : style + (long)(y - P) * HW) + lo;
    float mean = 0.0f, m2 = 0.0f;
    if (n > 0) {                                                      // (uniform over the workgroup)
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        if (vec) {
            for (int q = tid; q < n / 4; q += 256) {
                const f32x4 v = ((const f32x4*)x)[q];
                a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
            }
        } else {
            for (int i = tid; i < n; i += 1024) {
                a0 += x[i];
                if (i + 256 < n) a1 += x[i + 256];
                if (i + 512 < n) a2 += x[i + 512];
                if (i + 768 < n) a3 += x[i + 768];
            }
        }
        mean = block_sum((a0 + a1) + (a2 + a3), red) / (float)n;
        a0 = a1 = a2 = a3 = 0.0f;
        if (vec) {
            for (int q = tid; q < n / 4; q += 256) {
                const f32x4 v = ((const f32x4*)x)[q] - mean;
                a0 += v[0] * v[0]; a1 += v[1] * v[1]; a2 += v[2] * v[2]; a3 += v[3] * v[3];
            }
        } else {
            for (int i = tid; i < n; i += 1024) {
                float t = x[i] - mean;
                a0 += t * t;
                if (i + 256 < n) { t = x[i + 256] - mean; a1 += t * t; }
                if (i + 512 < n) { t = x[i + 512] - mean; a2 += t * t; }
                if (i + 768 < n) { t = x[i + 768] - mean; a3 += t * t; }
            }
        }
        m2 = block_sum((a0 + a1) + (a2 + a3), red);
    }
    if (tid == 0) {
        float* p = part + ((long)y * NSLAB + slab) * 3;
        p[0] = (float)n; p[1] = mean; p[2] = m2;
    }
}

// grid (ceil(HW / APPLY_ELEMS), P), 256 threads
__global__ __launch_bounds__(256) void adain_apply_kernel(const float* content, float* out, int HW, int P, const float* part, int vec) {
    __shared__ float st[4];                                          // mean_c std_c mean_s std_s
    __shared__ double red[2][NSLAB], tot[2][2];
    const int tid = threadIdx.x, y = blockIdx.y;
    // merge of the slab partials (content: threads 0..63, style: 64..127, one slab each), every sum taken in slab order:
    // N = sum n_i, mean = sum n_i m_i / N, M2 = sum (M2_i + n_i (m_i - mean)^2), in double
    const int which = tid >> 6, sl = tid & (NSLAB - 1);
    double nb = 0.0, mb = 0.0, qb = 0.0;
    if (tid < 2 * NSLAB) {
        const float* p = part + ((long)(y + which * P) * NSLAB + sl) * 3;
        nb = p[0]; mb = p[1]; qb = p[2];
        red[which][sl] = nb * mb;
    }
    __syncthreads();
    if (tid < 2 * NSLAB && sl == 0) {
        double a = 0.0;
        for (int i = 0; i < NSLAB; ++i) a += red[which][i];
        tot[which][0] = a / (double)HW;
    }
    __syncthreads();
    if (tid < 2 * NSLAB) {
        const double delta = mb - tot[which][0];
        red[which][sl] = qb + nb * delta * delta;
    }
    __syncthreads();
    if (tid < 2 * NSLAB && sl == 0) {
        double a = 0.0;
        for (int i = 0; i < NSLAB; ++i) a += red[which][i];
        st[2 * which] = (float)tot[which][0];
        st[2 * which + 1] = sqrtf((float)(a / ((double)HW - 1.0)) + 1e-5f);
    }
    __syncthreads();
    const float mc = st[0], sc = st[1], ms = st[2], ss = st[3];
    const long base = (long)y * HW;
    const int e0 = blockIdx.x * APPLY_ELEMS, e1 = min(e0 + APPLY_ELEMS, HW);
    if (vec) {
        for (int e = e0 + 4 * tid; e < e1; e += 1024) {
            const f32x4 v = *(const f32x4*)(content + base + e);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = clamp01((v[j] - mc) / sc * ss + ms);
            *(f32x4*)(out + base + e) = o;
        }
    } else {
        for (int e = e0 + tid; e < e1; e += 256) out[base + e] = clamp01((content[base + e] - mc) / sc * ss + ms);
    }
}

// planes of a (B, C, H, W) fp32 tensor, or -1
long cf_planes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return -1;
    const int64_t P = (int64_t)B * C;
    if (P > 32767) return -1;                                        // grid.z / 2 * P in grid.y
    return (long)P;
}

bool aligned16(const void* a, const void* b, const void* c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

extern "C" int64_t iir_colorfix_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    const long P = cf_planes(B, C, H, W);
    if (P < 0) return -1;
    const int64_t wavelet = (int64_t)P * H * W * (int64_t)sizeof(float);
    const int64_t adain = 2 * (int64_t)P * NSLAB * 3 * (int64_t)sizeof(float);
    return wavelet > adain ? wavelet : adain;
}

extern "C" int iir_colorfix_wavelet_f32(const float* content, const float* style, float* out, int32_t B, int32_t C, int32_t H,
                                        int32_t W, void* ws, int64_t ws_bytes, void* stream) {
    const long P = cf_planes(B, C, H, W);
    if (!content || !style || !out || !ws || P < 0) return IIR_EINVAL;
    if (ws_bytes < iir_colorfix_workspace_bytes(B, C, H, W)) return IIR_EINVAL;
    if ((int64_t)P * H > 0x7fffffffLL) return IIR_EINVAL;
    (void)hipGetLastError();
    const int w4 = W % 4 == 0;
    hipLaunchKernelGGL(wavelet_rows_kernel, dim3((unsigned)(P * H), (W + SEG - 1) / SEG), dim3(256), 0, (hipStream_t)stream, content,
                       style, (float*)ws, W, (int)(w4 && W <= SEG && aligned16(content, style, ws)));
    hipLaunchKernelGGL(wavelet_cols_kernel, dim3((W + TW - 1) / TW, (H + TH - 1) / TH, (unsigned)P), dim3(256), 0, (hipStream_t)stream,
                       content, (const float*)ws, out, H, W, (int)(w4 && aligned16(content, out, ws)));
    return iir_launch_status();
}

extern "C" int iir_colorfix_adain_f32(const float* content, const float* style, float* out, int32_t B, int32_t C, int32_t H,
                                      int32_t W, void* ws, int64_t ws_bytes, void* stream) {
    const long P = cf_planes(B, C, H, W);
    if (!content || !style || !out || !ws || P < 0) return IIR_EINVAL;
    if ((int64_t)H * W < 2 || (int64_t)H * W > (1 << 30)) return IIR_EINVAL;
    if (ws_bytes < iir_colorfix_workspace_bytes(B, C, H, W)) return IIR_EINVAL;
    (void)hipGetLastError();
    const int HW = H * W;
    const int h4 = HW % 4 == 0;
    hipLaunchKernelGGL(adain_stats_kernel, dim3(NSLAB, (unsigned)(2 * P)), dim3(256), 0, (hipStream_t)stream, content, style, HW, (int)P,
                       (float*)ws, (int)(h4 && aligned16(content, style, nullptr)));
    hipLaunchKernelGGL(adain_apply_kernel, dim3((HW + APPLY_ELEMS - 1) / APPLY_ELEMS, (unsigned)P), dim3(256), 0, (hipStream_t)stream,
                       content, out, HW, (int)P, (const float*)ws, (int)(h4 && aligned16(content, out, nullptr)));
    return iir_launch_status();
}
