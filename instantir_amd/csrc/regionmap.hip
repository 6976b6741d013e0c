// Region-selective restoration, the two pixel-space halves of a restore map (no reference counterpart; contract in
// include/instantir_hip.h and DESIGN.md section 7 "Restore map").  fp32 planar tensors, compiled with -ffp-contract=off like
// pointwise.hip and colorfix.hip.
//
// pool:      out[b][yo][xo] = max of map[b] over the factor x factor block under latent pixel (yo, xo): a latent pixel is
//            free if any pixel under it asked for freedom.
// composite: P = [map > 0]; cnt = sum of P over the (2r+1) x (2r+1) window with coordinates clamped to the image;
//            out = decoded where cnt == (2r+1)^2, original where cnt == 0, else w * decoded + (1 - w) * original with
//            w = cnt / (2r+1)^2.  Two separable passes on INTEGER counts: count_rows_kernel leaves the horizontal window
//            sums in the workspace (uint16, <= 2r+1), composite_cols_kernel adds 2r+1 of them vertically (a sliding window
//            down a strip of rows) and applies the formula to every channel.  The two ends are integer compares, so a pixel
//            whose window lies wholly in the kept region is the input pixel bit for bit, and one whose window lies wholly in
//            the free region is the decoded pixel.  No atomics: equal inputs give equal bits.
// Every load is unconditional, from a clamped address; only stores are guarded.
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int RMAX = IIR_REGION_MAX_FEATHER;
constexpr int SEG = 1024;                     // row pass: outputs of one row per workgroup
constexpr int NBUF = SEG + 2 * RMAX;          // flags of [s0 - r, s0 + SEG + r)
constexpr int CHUNK = NBUF / 256;             // flags one thread loads, and then sums on its own
constexpr int TH = 16;                        // column pass: rows per thread (one sliding window)
constexpr int STRIPS = 4;                     // strips per workgroup: 64 columns x (STRIPS * TH) rows
static_assert(NBUF % 256 == 0 && CHUNK == 8, "every thread of the row pass owns CHUNK flags, read as one 8-byte LDS load");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// V consecutive elements as one load / store (V = 4: the 16-byte and 8-byte forms; the host checks W % 4 and the alignment)
template <int V, typename T>
__device__ __forceinline__ void ldv(T (&dst)[V], const T* p) { __builtin_memcpy(dst, __builtin_assume_aligned(p, sizeof(T) * V), sizeof(T) * V); }
template <int V, typename T>
__device__ __forceinline__ void stv(T* p, const T (&src)[V]) { __builtin_memcpy(__builtin_assume_aligned(p, sizeof(T) * V), src, sizeof(T) * V); }

// grid (ceil(Wo * Ho * B / 256)), one thread per output.  V = 4: factor % 4 == 0, 16-byte aligned map.
template <int V>
__global__ __launch_bounds__(256) void pool_max_kernel(const float* map, int Ho, int Wo, int factor, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const long b = i / ((long)Wo * Ho);
    const long W = (long)Wo * factor;
    const float* src = map + (b * Ho * factor + (long)yo * factor) * W + (long)xo * factor;
    float m = src[0];
    for (int dy = 0; dy < factor; ++dy)
        for (int dx = 0; dx < factor; dx += V) {
            float v[V];
            ldv<V>(v, src + dy * W + dx);
#pragma unroll
            for (int j = 0; j < V; ++j) m = fmaxf(m, v[j]);
        }
    out[i] = m;
}

// grid (B * H, ceil(W / SEG)), 256 threads.  Flag k of the workgroup is P at column clamp(s0 - r + k): the window of output
// x is flags [x - s0, x - s0 + 2r], a difference of two entries of the exclusive prefix sum `pre`.
__global__ __launch_bounds__(256) void count_rows_kernel(const float* map, int W, int r, unsigned short* cnt) {
    __shared__ __attribute__((aligned(8))) unsigned char flag[NBUF];
    __shared__ int pre[NBUF + 1];
    __shared__ int tot[256];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * W;
    const int s0 = blockIdx.y * SEG, s1 = min(s0 + SEG, W);
    const int n = (s1 - s0) + 2 * r;                                  // flags in use
#pragma unroll
    for (int j = 0; j < CHUNK; ++j) {                                 // consecutive lanes, consecutive columns
        const int k = tid + 256 * j;
        unsigned char f = 0;
        if (256 * j < n) f = (map[row + clampi(s0 - r + k, 0, W - 1)] > 0.f && k < n) ? 1 : 0;      // (uniform over the workgroup)
        flag[k] = f;
    }
    __syncthreads();
    unsigned char local[CHUNK];
    ldv<CHUNK>(local, &flag[tid * CHUNK]);
    int sum = 0;
#pragma unroll
    for (int j = 0; j < CHUNK; ++j) sum += local[j];
    tot[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                               // inclusive scan of the 256 chunk sums
        const int add = tid >= o ? tot[tid - o] : 0;
        __syncthreads();
        tot[tid] += add;
        __syncthreads();
    }
    int run = tot[tid] - sum;                                         // flags before this thread's chunk
#pragma unroll
    for (int j = 0; j < CHUNK; ++j) {
        pre[tid * CHUNK + j] = run;
        run += local[j];
    }
    if (tid == 255) pre[NBUF] = run;
    __syncthreads();
    for (int x = s0 + tid; x < s1; x += 256) cnt[row + x] = (unsigned short)(pre[x - s0 + 2 * r + 1] - pre[x - s0]);
}

// grid (ceil(W / (64 V)), ceil(H / (STRIPS * TH)), B), block (64, STRIPS); a thread owns V adjacent columns of a strip of TH
// rows.  V = 4: W % 4 == 0 and aligned bases.  `out` may be `decoded`: every element is read, then written, by the one thread
// that owns it.
template <int V>
__global__ __launch_bounds__(64 * STRIPS) void composite_cols_kernel(const float* decoded, const float* original,
                                                                     const unsigned short* cnt, int C, int H, int W, int r,
                                                                     float* out) {
    const int x = (blockIdx.x * 64 + threadIdx.x) * V;
    const int xc = min(x, W - V);                                     // columns past W load the last ones and store nothing
    const int y0 = (blockIdx.y * STRIPS + threadIdx.y) * TH;
    if (y0 >= H) return;
    const int y1 = min(y0 + TH, H);
    const long b = blockIdx.z;
    const unsigned short* col = cnt + b * H * W + xc;
    const int full = (2 * r + 1) * (2 * r + 1);
    int s[V];
    unsigned short in[V], gone[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0;
    for (int dy = -r; dy <= r; ++dy) {
        ldv<V>(in, col + (long)clampi(y0 + dy, 0, H - 1) * W);
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] += in[j];
    }
    for (int y = y0; y < y1; ++y) {
        for (int c = 0; c < C; ++c) {
            const long m = ((b * C + c) * H + y) * W + xc;
            float d[V], o[V], v[V];
            ldv<V>(d, decoded + m);
            ldv<V>(o, original + m);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float w = (float)s[j] / (float)full;
                v[j] = s[j] == full ? d[j] : s[j] == 0 ? o[j] : w * d[j] + (1.0f - w) * o[j];
            }
            if (x < W) stv<V>(out + m, v);
        }
        ldv<V>(in, col + (long)clampi(y + 1 + r, 0, H - 1) * W);
        ldv<V>(gone, col + (long)clampi(y - r, 0, H - 1) * W);
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] += (int)in[j] - (int)gone[j];
    }
}

bool aligned16(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

// a (B, H, W) map inside the limits colorfix.hip sets for its planes
bool map_geometry_ok(int32_t B, int32_t H, int32_t W) {
    return B > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && B <= 32767 && (int64_t)B * H <= 0x7fffffffLL;
}

}  // namespace

extern "C" int iir_map_pool_max_f32(const float* map_px, int32_t B, int32_t H, int32_t W, int32_t factor, float* out, void* stream) {
    if (!map_px || !out || out == map_px || !map_geometry_ok(B, H, W)) return IIR_EINVAL;
    if (factor <= 0 || H % factor || W % factor) return IIR_EINVAL;
    const int Ho = H / factor, Wo = W / factor;
    const long n = (long)B * Ho * Wo;
    if ((n + 255) / 256 > 0x7fffffffL) return IIR_EINVAL;
    (void)hipGetLastError();
    const bool vec = factor % 4 == 0 && aligned16(map_px, nullptr, nullptr);
    hipLaunchKernelGGL(vec ? pool_max_kernel<4> : pool_max_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       map_px, Ho, Wo, factor, n, out);
    return iir_launch_status();
}

extern "C" int64_t iir_region_composite_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (!map_geometry_ok(B, H, W)) return -1;
    return (int64_t)B * H * W * (int64_t)sizeof(unsigned short);
}

extern "C" int iir_region_composite_f32(const float* decoded, const float* original, const float* map_px, int32_t B, int32_t C,
                                        int32_t H, int32_t W, int32_t r, void* ws, int64_t ws_bytes, float* out, void* stream) {
    if (!decoded || !original || !map_px || !ws || !out || !map_geometry_ok(B, H, W)) return IIR_EINVAL;
    if (C <= 0 || (int64_t)B * C > 32767 || r < 0 || r > RMAX) return IIR_EINVAL;
    if (out == original || out == map_px || (const void*)out == ws) return IIR_EINVAL;
    if (ws_bytes < iir_region_composite_workspace_bytes(B, H, W)) return IIR_EINVAL;
    if ((H + STRIPS * TH - 1) / (STRIPS * TH) > 65535) return IIR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(count_rows_kernel, dim3((unsigned)((int64_t)B * H), (W + SEG - 1) / SEG), dim3(256), 0, (hipStream_t)stream, map_px,
                       W, r, (unsigned short*)ws);
    const int V = (W % 4 == 0 && aligned16(decoded, original, out) && ((uintptr_t)ws & 7) == 0) ? 4 : 1;
    hipLaunchKernelGGL(V == 4 ? composite_cols_kernel<4> : composite_cols_kernel<1>,
                       dim3((W + 64 * V - 1) / (64 * V), (H + STRIPS * TH - 1) / (STRIPS * TH), (unsigned)B), dim3(64, STRIPS), 0,
                       (hipStream_t)stream, decoded, original, (const unsigned short*)ws, C, H, W, r, out);
    return iir_launch_status();
}
