// Synthetic degradation on the device: the three operations of the Real-ESRGAN second-order chain the tree lacked (the
// reference's utils/degradation_pipeline.py runs them through basicsr: filter2D, random_add_gaussian_noise_pt, DiffJPEG).
// Contracts in include/instantir_hip.h (iir_filter2d_f32, iir_add_gaussian_noise_f32, iir_jpeg_roundtrip_f32) and DESIGN.md
// section 7 "Synthetic degradation".  fp32 planar (N, C, H, W) images in [0, 1].  Compiled with -ffp-contract=off like
// metrics.hip: the sums are written with fmaf, so they are fused by statement and nothing else is.
//
// Every global load is unconditional, from an address clamped into the tensor; only stores are
// guarded.  No atomics, no scratch, every sum in a fixed order: equal inputs give equal bits.
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------------------------- filter2d
// The tiled form of lqfidelity.hip.  A workgroup owns a FT x FT output tile of one plane: it stages the tile plus the halo of
// the k x k window (reflected at the image's borders) and the image's taps in LDS; a thread owns FQ consecutive rows of one
// column and walks the staged rows of its column strip once: a staged pixel read from LDS feeds up to FQ accumulators, a tap
// read is a wave-wide broadcast.  (Taps read through the scalar cache instead -- a uniform address -- measured a third
// slower: DESIGN.md section 7.)  Each output's sum still runs over i (outer) and j (inner) in index order with fmaf from 0.
// A wave's 32-lane half reads 32 consecutive floats of one staged row: no pitch can make that conflict.
constexpr int KMAX = IIR_FILTER2D_MAX_KSIZE, RMAX = (KMAX - 1) / 2;
constexpr int FT = IIR_FILTER2D_TILE;
constexpr int FS = FT + 2 * RMAX;                   // staged rows and columns at the largest window
constexpr int FQ = FT / (NT / FT);                  // outputs per thread: 4 consecutive rows
static_assert(NT % FT == 0 && FQ * (NT / FT) == FT, "a thread owns FQ rows of one column");
static_assert((FS * FS + KMAX * KMAX) * sizeof(float) <= 48 * 1024, "static LDS");

__device__ __forceinline__ int reflecti(int t, int L) {
    t = t < 0 ? -t : t;
    t = t >= L ? 2 * (L - 1) - t : t;
    return clampi(t, 0, L - 1);       // only a row or column of a tile's part past the image needs the clamp; it is never stored
}

// grid (ceil(W / FT), ceil(H / FT), N * C), NT threads
__global__ __launch_bounds__(NT) void filter2d_kernel(const float* in, const float* taps, int C, int H, int W, int k, float* out) {
    __shared__ float sp[FS * FS];
    __shared__ float st[KMAX * KMAX];
    const int tid = threadIdx.x, tx = tid % FT, ty = (tid / FT) * FQ;
    const int tx0 = blockIdx.x * FT, ty0 = blockIdx.y * FT;
    const int r = (k - 1) / 2, SW = FT + 2 * r;
    const int n = blockIdx.z / C;
    const float* plane = in + (long)blockIdx.z * H * W;
    const float* kt = taps + (long)n * k * k;

    for (int i = tid; i < SW * SW; i += NT) {
        const int ly = i / SW, lx = i - ly * SW;
        sp[i] = plane[(long)reflecti(ty0 - r + ly, H) * W + reflecti(tx0 - r + lx, W)];
    }
    for (int i = tid; i < k * k; i += NT) st[i] = kt[i];
    __syncthreads();

    float acc[FQ];
#pragma unroll
    for (int q = 0; q < FQ; ++q) acc[q] = 0.0f;
    // staged row m of the thread's strip is row i = m - q of the window of output q
    for (int m = 0; m < k + FQ - 1; ++m) {
        const float* row = sp + (ty + m) * SW + tx;
        for (int j = 0; j < k; ++j) {
            const float p = row[j];
#pragma unroll
            for (int q = 0; q < FQ; ++q) {
                const int i = m - q;
                if (i >= 0 && i < k) acc[q] = fmaf(st[i * k + j], p, acc[q]);
            }
        }
    }
    float* oplane = out + (long)blockIdx.z * H * W;
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        const int gy = ty0 + ty + q, gx = tx0 + tx;
        if (gy < H && gx < W) oplane[(long)gy * W + gx] = acc[q];
    }
}

// ------------------------------------------------------------------------------------------------------------------- noise
struct U4 { uint32_t a, b, c, d; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.a), lo0 = 0xD2511F53u * c.a;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.c), lo1 = 0xCD9E8D57u * c.c;
        c = {hi1 ^ c.b ^ k0, lo1, hi0 ^ c.d ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// grid (ceil(N * C * H * W / NT)), NT threads: one thread per element
__global__ __launch_bounds__(NT) void noise_kernel(const float* in, const float* sigma, long total, int C, long HW, uint32_t k0,
                                                   uint32_t k1, uint32_t stream_id, int gray, float* out) {
    const long e = (long)blockIdx.x * NT + threadIdx.x, ec = min(e, total - 1);
    const long pl = ec / HW;                           // n * C + c
    const uint32_t pos = (uint32_t)(ec - pl * HW);     // y * W + x
    const uint32_t n = (uint32_t)(pl / C), ch = (uint32_t)(pl - (long)n * C);
    const float v = in[ec], s = sigma[n] / 255.0f;
    const U4 rnd = philox4x32_10({pos, n, gray ? 0u : ch, stream_id}, k0, k1);
    // (r >> 8) + 0.5 has 25 significant bits from 2^23 on and rounds to even there; the product with 2^-24 is exact
    const float u1 = ((float)(rnd.a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(rnd.b >> 8) + 0.5f) * 0x1p-24f;
    const float z = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
    const float o = fminf(fmaxf(v + s * z, 0.0f), 1.0f);
    if (e < total) out[e] = o;
}

// -------------------------------------------------------------------------------------------------------------------- JPEG
// One wave per 16 x 16 MCU, four MCUs per workgroup; lane = (row, column) = (lane / 8, lane % 8) of an 8 x 8 block.  A lane
// loads its pixel of each of the four luma blocks, the 2 x 2 chroma means and the replicated chroma go through LDS, and the
// six blocks (Y00, Y01, Y10, Y11, Cb, Cr) take the transform round trip in turn.  Each 8-point pass: one lane writes its value
// to the wave's 8 x 8 LDS image, reads the 8 values of its row (or column) back and sums basis * value over k = 0..7 in index
// order with fmaf from 0.  Two LDS images alternate, one workgroup barrier between a write and the reads of it.
//   forward:  t[y][v] = sum_x D[v][x] X[y][x]   then   c[u][v] = sum_y D[u][y] t[y][v]
//   inverse:  s[u][x] = sum_v D[v][x] c'[u][v]  then   X'[y][x] = sum_u D[u][y] s[u][x]
// D[u][k] = a(u) cos((2k + 1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2: formed in fp64, rounded to fp32.
__constant__ float DCT8[64] = {
    0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f,
    0x1.f6297cp-2f, 0x1.a9b662p-2f, 0x1.1c73b4p-2f, 0x1.8f8b84p-4f, -0x1.8f8b84p-4f, -0x1.1c73b4p-2f, -0x1.a9b662p-2f, -0x1.f6297cp-2f,
    0x1.d906bcp-2f, 0x1.87de2ap-3f, -0x1.87de2ap-3f, -0x1.d906bcp-2f, -0x1.d906bcp-2f, -0x1.87de2ap-3f, 0x1.87de2ap-3f, 0x1.d906bcp-2f,
    0x1.a9b662p-2f, -0x1.8f8b84p-4f, -0x1.f6297cp-2f, -0x1.1c73b4p-2f, 0x1.1c73b4p-2f, 0x1.f6297cp-2f, 0x1.8f8b84p-4f, -0x1.a9b662p-2f,
    0x1.6a09e6p-2f, -0x1.6a09e6p-2f, -0x1.6a09e6p-2f, 0x1.6a09e6p-2f, 0x1.6a09e6p-2f, -0x1.6a09e6p-2f, -0x1.6a09e6p-2f, 0x1.6a09e6p-2f,
    0x1.1c73b4p-2f, -0x1.f6297cp-2f, 0x1.8f8b84p-4f, 0x1.a9b662p-2f, -0x1.a9b662p-2f, -0x1.8f8b84p-4f, 0x1.f6297cp-2f, -0x1.1c73b4p-2f,
    0x1.87de2ap-3f, -0x1.d906bcp-2f, 0x1.d906bcp-2f, -0x1.87de2ap-3f, -0x1.87de2ap-3f, 0x1.d906bcp-2f, -0x1.d906bcp-2f, 0x1.87de2ap-3f,
    0x1.8f8b84p-4f, -0x1.1c73b4p-2f, 0x1.a9b662p-2f, -0x1.f6297cp-2f, 0x1.f6297cp-2f, -0x1.a9b662p-2f, 0x1.1c73b4p-2f, -0x1.8f8b84p-4f,
};
// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance); row = vertical frequency
__constant__ float QTAB[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

struct Basis {
    float row[8];       // D[lane % 8][k]: the forward pass along x
    float col[8];       // D[lane / 8][k]: the forward pass along y
    float rowT[8];      // D[k][lane % 8]: the inverse pass along v
    float colT[8];      // D[k][lane / 8]: the inverse pass along u
};

// v = sample - 128 of this lane -> the sample after DCT, quantisation with `step`, dequantisation and inverse DCT, + 128
__device__ __forceinline__ float block_roundtrip(float v, float step, const Basis& d, float* a, float* b, int lr, int lc) {
    const int me = lr * 8 + lc;
    a[me] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t = fmaf(d.row[k], a[lr * 8 + k], t);
    b[me] = t;
    __syncthreads();
    float c = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = fmaf(d.col[k], b[k * 8 + lc], c);
    const float qc = rintf(c / step);
    a[me] = qc * step;
    __syncthreads();
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf(d.rowT[k], a[lr * 8 + k], s);
    b[me] = s;
    __syncthreads();
    float x = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) x = fmaf(d.colT[k], b[k * 8 + lc], x);
    return x + 128.0f;
}

// grid (ceil(mcus / 4), N), NT threads; mcus = ceil(H / 16) * ceil(W / 16) per image, row-major
__global__ __launch_bounds__(NT) void jpeg_kernel(const float* in, const float* quality, int H, int W, int mw, int mcus, float* out) {
    __shared__ float sa[4][64], sb[4][64];              // the two 8 x 8 images of each wave's passes
    __shared__ float scb[4][256], scr[4][256];          // Cb, Cr of the wave's MCU before the 2 x 2 mean; 64 of each after the round trip
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane >> 3, lc = lane & 7;
    const int mcu = blockIdx.x * 4 + wv;
    const bool live = mcu < mcus;
    const int mc = min(mcu, mcus - 1);                  // a surplus wave repeats the last MCU and stores nothing
    const int my = mc / mw, mx = mc - my * mw;
    const int n = blockIdx.y;
    const long HW = (long)H * W;
    const float* img = in + (long)n * 3 * HW;

    Basis d;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        d.row[k] = DCT8[lc * 8 + k];
        d.col[k] = DCT8[lr * 8 + k];
        d.rowT[k] = DCT8[k * 8 + lc];
        d.colT[k] = DCT8[k * 8 + lr];
    }
    float q = quality[n];
    q = fminf(fmaxf(q, 1.0f), 99.0f);
    const float f = (q < 50.0f ? 5000.0f / q : 200.0f - 2.0f * q) / 100.0f;
    const float step_y = QTAB[0][lr * 8 + lc] * f, step_c = QTAB[1][lr * 8 + lc] * f;

    float Y[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int py = 8 * (b >> 1) + lr, px = 8 * (b & 1) + lc;                      // inside the MCU
        const long o = (long)min(my * 16 + py, H - 1) * W + min(mx * 16 + px, W - 1);    // edge replication
        float R = img[o], G = img[o + HW], B = img[o + 2 * HW];
        R = 255.0f * fminf(fmaxf(R, 0.0f), 1.0f);
        G = 255.0f * fminf(fmaxf(G, 0.0f), 1.0f);
        B = 255.0f * fminf(fmaxf(B, 0.0f), 1.0f);
        Y[b] = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R));
        scb[wv][py * 16 + px] = fmaf(0.5f, B, fmaf(-0.331264f, G, -0.168736f * R)) + 128.0f;
        scr[wv][py * 16 + px] = fmaf(-0.081312f, B, fmaf(-0.418688f, G, 0.5f * R)) + 128.0f;
    }
    __syncthreads();
    const int c00 = 2 * lr * 16 + 2 * lc;
    const float cb = ((scb[wv][c00] + scb[wv][c00 + 1]) + (scb[wv][c00 + 16] + scb[wv][c00 + 17])) * 0.25f;
    const float cr = ((scr[wv][c00] + scr[wv][c00 + 1]) + (scr[wv][c00 + 16] + scr[wv][c00 + 17])) * 0.25f;

#pragma unroll
    for (int b = 0; b < 4; ++b) Y[b] = block_roundtrip(Y[b] - 128.0f, step_y, d, sa[wv], sb[wv], lr, lc);
    const float cb2 = block_roundtrip(cb - 128.0f, step_c, d, sa[wv], sb[wv], lr, lc);
    const float cr2 = block_roundtrip(cr - 128.0f, step_c, d, sa[wv], sb[wv], lr, lc);
    // every lane read its four means before the first barrier of the round trips: the front of scb / scr is free
    scb[wv][lr * 8 + lc] = cb2;
    scr[wv][lr * 8 + lc] = cr2;
    __syncthreads();

    float* oimg = out + (long)n * 3 * HW;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int py = 8 * (b >> 1) + lr, px = 8 * (b & 1) + lc;
        const int ci = (py >> 1) * 8 + (px >> 1);                                       // replication
        const float db = scb[wv][ci] - 128.0f, dr = scr[wv][ci] - 128.0f;
        const float R = fmaf(1.402f, dr, Y[b]);
        const float G = fmaf(-0.714136f, dr, fmaf(-0.344136f, db, Y[b]));
        const float B = fmaf(1.772f, db, Y[b]);
        const int gy = my * 16 + py, gx = mx * 16 + px;
        if (live && gy < H && gx < W) {
            const long o = (long)gy * W + gx;
            oimg[o] = fminf(fmaxf(R, 0.0f), 255.0f) / 255.0f;
            oimg[o + HW] = fminf(fmaxf(G, 0.0f), 255.0f) / 255.0f;
            oimg[o + 2 * HW] = fminf(fmaxf(B, 0.0f), 255.0f) / 255.0f;
        }
    }
}

bool overlap(const void* a, const void* b, int64_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace

extern "C" int iir_filter2d_f32(const float* in, const float* taps, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ksize, float* out,
                                void* stream) {
    if (!in || !taps || !out) return IIR_EINVAL;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || (int64_t)N * C > 65535) return IIR_EINVAL;
    if (ksize < 1 || ksize > KMAX || !(ksize & 1)) return IIR_EINVAL;
    const int r = (ksize - 1) / 2;
    if (H <= r || W <= r) return IIR_EINVAL;
    // neighbours read `in` through their halos
    if (overlap(in, out, (int64_t)N * C * H * W * (int64_t)sizeof(float))) return IIR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(filter2d_kernel, dim3((W + FT - 1) / FT, (H + FT - 1) / FT, (unsigned)(N * C)), dim3(NT), 0, (hipStream_t)stream, in,
                       taps, (int)C, (int)H, (int)W, (int)ksize, out);
    return iir_launch_status();
}

extern "C" int iir_add_gaussian_noise_f32(const float* in, const float* sigma, int32_t N, int32_t C, int32_t H, int32_t W, uint64_t seed,
                                          uint32_t noise_stream, int32_t gray, float* out, void* stream) {
    if (!in || !sigma || !out) return IIR_EINVAL;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return IIR_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (HW >= (1LL << 32)) return IIR_EINVAL;
    const int64_t total = (int64_t)N * C * HW;
    if ((total + NT - 1) / NT > 0x7fffffffLL) return IIR_EINVAL;
    // pointwise: out may be in, but not a shifted view of it
    if (out != in && overlap(in, out, total * (int64_t)sizeof(float))) return IIR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, in, sigma, (long)total, (int)C,
                       (long)HW, (uint32_t)seed, (uint32_t)(seed >> 32), noise_stream, (int)(gray != 0), out);
    return iir_launch_status();
}

extern "C" int iir_jpeg_roundtrip_f32(const float* in, const float* quality, int32_t N, int32_t C, int32_t H, int32_t W, float* out,
                                      void* stream) {
    if (!in || !quality || !out) return IIR_EINVAL;
    if (N <= 0 || N > 65535 || C != 3 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return IIR_EINVAL;
    // a wave reads the MCU it writes and nothing else, all of it before its first store: out may be in, but not a shifted view
    if (out != in && overlap(in, out, (int64_t)N * 3 * H * W * (int64_t)sizeof(float))) return IIR_EINVAL;
    const int mw = (W + 15) / 16, mh = (H + 15) / 16, mcus = mw * mh;
    (void)hipGetLastError();
    hipLaunchKernelGGL(jpeg_kernel, dim3((unsigned)((mcus + 3) / 4), (unsigned)N), dim3(NT), 0, (hipStream_t)stream, in, quality, (int)H,
                       (int)W, mw, mcus, out);
    return iir_launch_status();
}
