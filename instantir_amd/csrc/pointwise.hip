// K9 and layout glue: timestep sinusoid, SiLU, concat/copy with scaled add, latent pack/unpack,
// classifier-free guidance (plain, PAG, adaptive projected) + scheduler update, LCM one-step preview.  All HBM-bound pointwise work.
// Compiled with -ffp-contract=off: the scheduler arithmetic follows the reference's fp32 op order
// (no FMA contraction) so it can be compared with the CPU restatement at rounding level.
//
// Replaces: Timesteps (module/min_sdxl.py:205-224); nn.SiLU on temb (:263); torch.cat of skip tensors
// (:712) with the ControlNet residual add folded in (pipelines/sdxl_instantir.py:1602-1603 and diffusers'
// `skip + residual`); latent_model_input = cat([latents]*2) (:1503); CFG (:1619-1621); main scheduler
// step (:1629-1633, DDPM / DDIM linear forms, and the Euler / Euler-ancestral / DPM++ 2M forms with one history
// plane); LCMSingleStepScheduler.step
// (schedulers/lcm_single_step_scheduler.py:455-484).
#include "common.h"
#include "../../include/instantir_hip.h"

namespace {

__global__ void sinusoid_kernel(const float* vals, int n_vals, int rows, int dim, f16* out, long ldo, int col_off) {
    // out[row][col_off + v*dim + (0..dim)] = [cos(val_v * w_k) | sin(val_v * w_k)], w_k = exp(-ln(1e4) k / (dim/2))
    // vals is [rows][n_vals] when rows_vals (vals per row), broadcast when n_vals rows == 1 handled by host.
    const int half = dim >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = rows * n_vals * half;
    if (idx >= total) return;
    const int k = idx % half;
    const int v = (idx / half) % n_vals;
    const int r = idx / (half * n_vals);
    const float w = expf(-9.210340371976184f * (float)k / (float)half);
    const float a = vals[r * n_vals + v] * w;
    f16* o = out + (long)r * ldo + col_off + v * dim;
    o[k] = (f16)cosf(a);
    o[half + k] = (f16)sinf(a);
}

__global__ void silu_kernel(const f16* x, f16* y, long n8) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const f16x8 v = *(const f16x8*)(x + i * 8);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)silu_f((float)v[j]);
    *(f16x8*)(y + i * 8) = o;
}

// dst[m][dst_off + c] = src[m][c] + add[m][c] * add_scale[m / rows_per_scale]   (add optional)
__global__ void copy_add_kernel(const f16* src, long lds_, f16* dst, long ldd, long dst_off, long M, int C, const f16* add,
                                long lda, const float* add_scale, int rows_per_scale) {
    const int nchunk = C >> 3;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * nchunk) return;
    const long m = i / nchunk;
    const int ch = (int)(i % nchunk);
    f16x8 v = *(const f16x8*)(src + m * lds_ + ch * 8);
    if (add) {
        const f16x8 a = *(const f16x8*)(add + m * lda + ch * 8);
        const float s = add_scale ? add_scale[m / rows_per_scale] : 1.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] + (float)a[j] * s);
    }
    *(f16x8*)(dst + m * ldd + dst_off + ch * 8) = v;
}

// fp32 NCHW (B, C, H, W) -> f16 NHWC rows (rep*B, H*W, ldo), channels [0,C) written, repeated `rep` times.  The scale is the
// host float, or read from `scale_dev` when given (sigma schedulers: the UNet input c_in * x changes every step, and a host
// float would be baked into a captured graph).  One product expression, so equal scales give equal bits.
template <typename E>
__global__ void pack_latent_kernel(const float* x, int B, int C, int HW, E* out, long ldo, int rep, float scale,
                                   const float* scale_dev) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * HW) return;
    if (scale_dev) scale = *scale_dev;
    const int b = (int)(i / HW), p = (int)(i % HW);
    for (int c = 0; c < C; ++c) {
        const E v = (E)(x[((long)b * C + c) * HW + p] * scale);
        for (int k = 0; k < rep; ++k) out[((long)(k * B + b) * HW + p) * ldo + c] = v;
    }
}

// f16 NHWC rows (R, H*W, ldi) channels [0,C) -> fp32 NCHW (R, C, H, W)
template <typename E>
__global__ void unpack_latent_kernel(const E* in, long ldi, int R, int C, int HW, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * HW) return;
    const int r = (int)(i / HW), p = (int)(i % HW);
    for (int c = 0; c < C; ++c) out[((long)r * C + c) * HW + p] = (float)in[((long)r * HW + p) * ldi + c];
}

// Main scheduler step with classifier-free guidance, fp32.
//   eps  = cfg ? u + g * (c - u) : c         (u = rows [0,B), c = rows [B,2B) of the UNet output)
//   x0   = (x - sqrt_beta_t * eps) / sqrt_alpha_t
//   prev = k_x0 * x0 + k_x * x + k_eps * eps + k_h * m_prev + k_noise * noise
// coef (device, fp32[8]) = {g, sqrt_beta_t, sqrt_alpha_t, k_x0, k_x, k_eps, k_noise, k_h}
// rescale_noise_cfg (pipelines/sdxl_instantir.py:181-192): per image, over (C, H, W),
//   factor = phi * std(eps_text) / std(eps_cfg) + (1 - phi),  eps_cfg = u + g * (text - u)   (torch.std: unbiased; the
// N-1 cancels in the ratio).  One workgroup per image, fp32 element math, fp64 accumulation.
// PAG (pag_s given): eps_cfg gains the perturbed-attention term + s * (text - perturbed) (rows [2B, 3B)), s = *pag_s, before
// the ratio.
__global__ __launch_bounds__(1024) void cfg_rescale_kernel(const f16* eps_nhwc, long lde, int B, int C, int HW, const float* coef,
                                                           const float* pag_s, float phi, float* factor) {
    __shared__ double red[4][16];
    const int b = blockIdx.x;
    const float g = coef[0];
    const float ps = pag_s ? *pag_s : 0.f;
    double st = 0., st2 = 0., sc = 0., sc2 = 0.;
    for (int p = threadIdx.x; p < HW; p += blockDim.x)
        for (int c = 0; c < C; ++c) {
            const float u = (float)eps_nhwc[((long)b * HW + p) * lde + c];
            const float t = (float)eps_nhwc[((long)(B + b) * HW + p) * lde + c];
            float e = u + g * (t - u);
            if (ps != 0.f) e = e + ps * (t - (float)eps_nhwc[((long)(2 * B + b) * HW + p) * lde + c]);
            st += t; st2 += (double)t * t; sc += e; sc2 += (double)e * e;
        }
    double v[4] = {st, st2, sc, sc2};
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 4; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if (lane == 0) red[k][wv] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        double s[4] = {0., 0., 0., 0.};
        for (int k = 0; k < 4; ++k)
            for (int w = 0; w < nw; ++w) s[k] += red[k][w];
        const double n = (double)C * HW;
        const double var_t = (s[1] - s[0] * s[0] / n) / (n - 1.), var_c = (s[3] - s[2] * s[2] / n) / (n - 1.);
        factor[b] = (float)((double)phi * sqrt(var_t / var_c) + (1. - (double)phi));
    }
}

// Adaptive projected guidance (APG, Sadat et al. 2024), the per-image half.  On denoised predictions, per image b over (C, H, W):
//   x0_c = (x - sb*c)/sa   x0_u = (x - sb*u)/sa   A = (x0_c - x0_u) + beta_t * A_prev
//   s = r > 0 ? min(1, r / ||A||) : 1            alpha = <A, x0_c> / <x0_c, x0_c>   (0 when x0_c is all zero)
// par (device fp32[4]) = {eta, r, beta_t, 0}; sb = coef[1], sa = coef[2].  `avg` (fp32 NCHW) holds A_prev on entry and A on exit: each
// element is read, then overwritten by the thread that owns it, and is never loaded when beta_t == 0 (uninitialised or stale
// on a call's first step: 0 * NaN would leak).  fp32 element math, fp64 accumulation.  Only columns [0, C) of rows [0, 2B) are read.
// An image is split over APG_PARTS workgroups (one alone is bound by what a single CU pulls through its L1: 133 us at 128 x 128
// with lde = 64): workgroup (part, b) owns a contiguous run of pixels and writes its three sums to ws[(b * APG_PARTS + part) * 3 ..]
// (zeros for an empty run); apg_finalize_kernel adds the APG_PARTS partials of an image in index order and writes
// out[2b] = s, out[2b + 1] = alpha.  Every order is fixed and there are no atomics: equal inputs give equal bits.
constexpr int APG_PARTS = 32, APG_THREADS = 256;

__global__ __launch_bounds__(APG_THREADS) void apg_project_kernel(const f16* eps_nhwc, long lde, int B, int C, int HW, const float* coef,
                                                                  const float* x, const float* par, float* avg, double* ws) {
    __shared__ double red[3][APG_THREADS / 64];
    const int part = blockIdx.x, b = blockIdx.y;
    const float sb = coef[1], sa = coef[2];
    const float beta = par[2];
    const int chunk = (HW + APG_PARTS - 1) / APG_PARTS;
    const int p0 = part * chunk, p1 = min(HW, p0 + chunk);
    double aa = 0., ac = 0., cc = 0.;
    for (int p = p0 + threadIdx.x; p < p1; p += APG_THREADS)
        for (int c = 0; c < C; ++c) {
            const long o = ((long)b * C + c) * HW + p;
            const float u = (float)eps_nhwc[((long)b * HW + p) * lde + c];
            const float t = (float)eps_nhwc[((long)(B + b) * HW + p) * lde + c];
            const float xv = x[o];
            const float x0c = (xv - sb * t) / sa;
            const float x0u = (xv - sb * u) / sa;
            float a = x0c - x0u;
            if (beta != 0.f) a = a + beta * avg[o];
            avg[o] = a;
            aa += (double)a * a; ac += (double)a * x0c; cc += (double)x0c * x0c;
        }
    double v[3] = {aa, ac, cc};
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 3; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if (lane == 0) red[k][wv] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.;
        for (int w = 0; w < APG_THREADS / 64; ++w) s += red[threadIdx.x][w];
        ws[((long)b * APG_PARTS + part) * 3 + threadIdx.x] = s;
    }
}

__global__ void apg_finalize_kernel(const double* ws, int B, const float* par, float* out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float r = par[1];
    double s[3] = {0., 0., 0.};
    for (int part = 0; part < APG_PARTS; ++part)
        for (int k = 0; k < 3; ++k) s[k] += ws[((long)b * APG_PARTS + part) * 3 + k];
    double sc = 1.;
    if (r > 0.f) sc = fmin(1., (double)r / sqrt(s[0]));
    out[2 * b] = (float)sc;
    out[2 * b + 1] = s[2] > 0. ? (float)(s[1] / s[2]) : 0.f;
}

// Perturbed-attention guidance (PAG) form: the UNet output has one more group of B rows, the perturbed prediction p
// (rows [2B, 3B) with CFG, [B, 2B) without), and  eps = u + g * (c - u) + s * (c - p)  (CFG) or  c + s * (c - p),  s = *pag_s
// (device: the per-step s_t of the adaptive scale).  The term is skipped when s == 0 (ps = 0 without PAG), so s = 0 gives
// the plain bits and the perturbed rows are never read.
// APG (apg_avg given, cfg only): u + g * (c - u) is replaced by the eps of the projected x0 guidance,
//   x0_c = (x - sb*c)/sa   U = s * (A - ((1 - eta) * alpha) * x0_c)   x0_g = x0_c + (g - 1) * U   eps = (x - sa*x0_g)/sb
// with A = apg_avg[o] and {s, alpha} = apg_sa[2b..] from apg_project_kernel, eta = apg_par[0]; the uncond rows are not read (A
// carries them).  The PAG term and eps_factor follow as without APG.
struct apg_lane {
    const float* avg = nullptr;
    float s = 0.f, k = 0.f, sb = 0.f, sa = 0.f;     // k = (1 - eta) * alpha
};

__device__ __forceinline__ float guided_eps(const f16* eps_nhwc, long lde, int B, int HW, int cfg, float g, float ps,
                                            const float* eps_factor, int b, int p, int c, const apg_lane& apg = {}, long o = 0,
                                            float xv = 0.f) {
    float e;
    if (cfg) {
        // the reference forms the guidance in the UNet dtype (fp16) -- keep fp32 here (>= precision)
        const float t = (float)eps_nhwc[((long)(B + b) * HW + p) * lde + c];
        if (apg.avg) {
            const float x0c = (xv - apg.sb * t) / apg.sa;
            const float up = apg.s * (apg.avg[o] - apg.k * x0c);
            const float x0g = x0c + (g - 1.f) * up;
            e = (xv - apg.sa * x0g) / apg.sb;
        } else {
            const float u = (float)eps_nhwc[((long)b * HW + p) * lde + c];
            e = u + g * (t - u);
        }
        if (ps != 0.f) e = e + ps * (t - (float)eps_nhwc[((long)(2 * B + b) * HW + p) * lde + c]);
        if (eps_factor) e *= eps_factor[b];
    } else {
        e = (float)eps_nhwc[((long)b * HW + p) * lde + c];
        if (ps != 0.f) e = e + ps * (e - (float)eps_nhwc[((long)(B + b) * HW + p) * lde + c]);
    }
    return e;
}

// The update of element o, written once for the NHWC and the fp32 step.  k = {sb, sa, k_x0, k_x, k_eps, k_noise, k_h}; a term
// whose coefficient is 0 is skipped.  hist (optional, multistep solvers such as DPM++ 2M) holds m_prev on entry and this
// step's x0 on exit: each element is read, then overwritten by the thread that owns it, so one captured launch serves every
// step.  With k_h == 0 the plane is never loaded (it is uninitialised or stale on a solver's first step, and 0 * NaN would
// leak into prev).
// a*x + b*y, the one expression behind add_noise (axpby_f32_kernel) and the kept value of a restore map (sched_step_kernel):
// equal arguments give equal bits in both.
__device__ __forceinline__ float axpby(float a, float x, float b, float y) { return a * x + b * y; }

// The value a kept element takes: add_noise(src, noise) with the pair (a, b); a term whose coefficient is 0 is skipped, so
// (1, 0) returns the bits of src whatever the noise plane holds.
__device__ __forceinline__ float keep_value(float a, float src, float b, float nz) {
    if (b == 0.f) return a * src;
    if (a == 0.f) return b * nz;
    return axpby(a, src, b, nz);
}

// (`kept`: the element takes `keep_v` instead of the update -- a select on the stored value only; x0 and hist are the model's.)
__device__ __forceinline__ void sched_update(float e, long o, const float (&k)[7], const float* x, const float* noise, float* hist,
                                             float* prev, float* x0_out, bool kept = false, float keep_v = 0.f) {
    const float xv = x[o];
    const float x0 = (xv - k[0] * e) / k[1];
    float pv = k[2] * x0 + k[3] * xv;
    if (k[4] != 0.f) pv = pv + k[4] * e;
    if (hist && k[6] != 0.f) pv = pv + k[6] * hist[o];
    if (noise && k[5] != 0.f) pv = pv + k[5] * noise[o];
    prev[o] = kept ? keep_v : pv;
    if (hist) hist[o] = x0;
    if (x0_out) x0_out[o] = x0;
}

// One thread per latent pixel; pag_s, noise, hist, x0_out, eps_out, eps_factor, the keep_* group and the apg_* group are optional
// (every branch on them is wave-uniform).  coef is read once, before the channel loop: prev may alias it as far as the compiler knows.
// keep_map (restore map, fp32 B x HW) with keep_coef = {thr, a, b, 0}: a pixel with map <= thr (fp32 compare) stores
// keep_value(a, keep_src, b, keep_noise) in prev instead of the update.  keep_src / keep_noise are loaded for every lane
// (no per-lane-predicated load); the per-lane part is the select alone, so a free element has the bits of the launch
// without a map and a kept one never sees its eps.
__global__ void sched_step_kernel(const f16* eps_nhwc, long lde, int B, int C, int HW, int cfg, const float* coef,
                                  const float* pag_s, const float* x, const float* noise, float* hist, float* prev,
                                  float* x0_out, float* eps_out, const float* eps_factor, const float* keep_map,
                                  const float* keep_src, const float* keep_noise, const float* keep_coef, const float* apg_avg,
                                  const float* apg_sa, const float* apg_par) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * HW) return;
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float g = coef[0];
    const float k[7] = {coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7]};
    const float ps = pag_s ? *pag_s : 0.f;
    apg_lane apg;
    if (apg_avg) {
        apg.avg = apg_avg; apg.s = apg_sa[2 * b]; apg.k = (1.f - apg_par[0]) * apg_sa[2 * b + 1];
        apg.sb = k[0]; apg.sa = k[1];
    }
    float ka = 0.f, kb = 0.f;
    bool kept = false;
    if (keep_map) {
        ka = keep_coef[1]; kb = keep_coef[2];
        kept = keep_map[(long)b * HW + p] <= keep_coef[0];
    }
    for (int c = 0; c < C; ++c) {
        const long o = ((long)b * C + c) * HW + p;
        const float e = apg_avg ? guided_eps(eps_nhwc, lde, B, HW, cfg, g, ps, eps_factor, b, p, c, apg, o, x[o])
                                : guided_eps(eps_nhwc, lde, B, HW, cfg, g, ps, eps_factor, b, p, c);
        const float kv = keep_map ? keep_value(ka, keep_src[o], kb, keep_noise[o]) : 0.f;
        sched_update(e, o, k, x, noise, hist, prev, x0_out, kept, kv);
        if (eps_out) eps_out[o] = e;
    }
}

// LCM one-step preview for every row of the CFG-doubled batch:
//   x0 = (x - sqrt_beta * eps) / sqrt_alpha ; den = c_out * x0 + c_skip * x
// coef (device fp32[4]) = {sqrt_beta, sqrt_alpha, c_out, c_skip}; x is the fp32 latent (B rows, shared by
// both CFG halves), eps the UNet output (R = rep*B rows, NHWC f16).  Writes f16 NHWC (R rows) and
// optionally fp32 NCHW (R rows).
__global__ void lcm_step_kernel(const f16* eps_nhwc, long lde, int B, int rep, int C, int HW, const float* coef,
                                const float* x, f16* out_nhwc, long ldo, float* out_nchw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * rep * HW) return;
    const int r = (int)(i / HW), p = (int)(i % HW);
    const int b = r % B;
    const float sb = coef[0], sa = coef[1], co = coef[2], cs = coef[3];
    for (int c = 0; c < C; ++c) {
        const float xv = x[((long)b * C + c) * HW + p];
        const float e = (float)eps_nhwc[((long)r * HW + p) * lde + c];
        const float x0 = (xv - sb * e) / sa;
        const float d = co * x0 + cs * xv;
        out_nhwc[((long)r * HW + p) * ldo + c] = (f16)d;
        if (out_nchw) out_nchw[((long)r * C + c) * HW + p] = d;
    }
}

// out[cols][rows_pad] = in[rows][cols]^T with zero fill of the row padding (one-time V^T builds)
__global__ void transpose_kernel(const f16* in, long ldi, int rows, int cols, f16* out, long ldo, int rows_pad) {
    __shared__ f16 tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;   // bx over cols, by over rows
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int r = by + j, c = bx + threadIdx.x;
        // unconditional load from a clamped address, then a select: no per-lane-predicated global_load (the form DESIGN.md 5.8 retires)
        const f16 v = in[(long)min(r, rows - 1) * ldi + min(c, cols - 1)];
        tile[j][threadIdx.x] = (r < rows && c < cols) ? v : (f16)0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = bx + j, r = by + threadIdx.x;
        if (c < cols && r < rows_pad) out[(long)c * ldo + r] = tile[threadIdx.x][j];
    }
}

// Batched 16-byte copies: job j of the device table {src, dst, units} copies `units` x 16 bytes (blockIdx.y = job).
__global__ void copy_segments_kernel(const long long* jobs) {
    const long long* jb = jobs + 3 * blockIdx.y;
    const long n = (long)jb[2];
    const uint4* src = (const uint4*)jb[0];
    uint4* dst = (uint4*)jb[1];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i];
}

inline int nblk(long n, int t) { return (int)((n + t - 1) / t); }

// One launcher per family: the validation the exported entries share is here, what an entry refuses on its own (a missing
// device scale) is in its forwarder below.
template <typename... A>
int launch_1d(void (*kern)(A...), long n, void* stream, A... args) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, args...);
    return iir_launch_status();
}

int launch_pack(const float* x, int B, int C, int HW, void* out, long ldo, int rep, float scale, const float* scale_dev, int dtype,
                void* stream) {
    if (!x || !out || B <= 0 || C <= 0 || HW <= 0 || rep <= 0 || ldo < C) return IIR_EINVAL;
    if (dtype == IIR_DT_BF16) return launch_1d(pack_latent_kernel<bf16>, (long)B * HW, stream, x, B, C, HW, (bf16*)out, ldo, rep, scale, scale_dev);
    if (dtype == IIR_DT_F16) return launch_1d(pack_latent_kernel<f16>, (long)B * HW, stream, x, B, C, HW, (f16*)out, ldo, rep, scale, scale_dev);
    return IIR_EINVAL;
}

int launch_unpack(const void* in, long ldi, int R, int C, int HW, float* out, int dtype, void* stream) {
    if (!in || !out || R <= 0 || C <= 0 || HW <= 0 || ldi < C) return IIR_EINVAL;
    if (dtype == IIR_DT_BF16) return launch_1d(unpack_latent_kernel<bf16>, (long)R * HW, stream, (const bf16*)in, ldi, R, C, HW, out);
    if (dtype == IIR_DT_F16) return launch_1d(unpack_latent_kernel<f16>, (long)R * HW, stream, (const f16*)in, ldi, R, C, HW, out);
    return IIR_EINVAL;
}

// hist, when given, is read and rewritten per element: it may not be one of the other planes
inline bool hist_aliases(const float* hist, const float* x, const float* prev, const float* x0_out) {
    return hist && (hist == x || hist == prev || hist == x0_out);
}

// pointers of an optional group against its bit in iir_sched_desc.groups: all given with the bit, none without it
inline bool group_ok(bool on, std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if (on != (q != nullptr)) return false;
    return true;
}

int launch_cfg_rescale(const iir_sched_desc* d, float phi, float* factor, void* stream) {
    if (!d || !d->eps_nhwc || !d->coef || !factor || d->B <= 0 || d->C <= 0 || d->HW <= 0 || d->lde < d->C || (long)d->C * d->HW < 2)
        return IIR_EINVAL;
    const float* pag_s = (d->groups & IIR_STEP_PAG) ? d->pag_scale : nullptr;
    if ((d->groups & IIR_STEP_PAG) && !pag_s) return IIR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3(d->B), dim3(1024), 0, (hipStream_t)stream, (const f16*)d->eps_nhwc, (long)d->lde, d->B,
                       d->C, d->HW, d->coef, pag_s, phi, factor);
    return iir_launch_status();
}

// Every refusal of the step, then the one place where the descriptor is spread into the kernel's arguments.
int launch_sched_step(const iir_sched_desc& d, void* stream) {
    if (!d.eps_nhwc || !d.coef || !d.x || !d.prev || d.B <= 0 || d.C <= 0 || d.HW <= 0 || d.lde < d.C) return IIR_EINVAL;
    if (d.eps_factor && !d.cfg) return IIR_EINVAL;
    const uint32_t g = d.groups;
    if (g & ~(IIR_STEP_PAG | IIR_STEP_HIST | IIR_STEP_KEEP | IIR_STEP_APG)) return IIR_EINVAL;
    if (!group_ok(g & IIR_STEP_PAG, {d.pag_scale}) || !group_ok(g & IIR_STEP_HIST, {d.hist}) ||
        !group_ok(g & IIR_STEP_KEEP, {d.keep_map, d.keep_src, d.keep_noise, d.keep_coef}) ||
        !group_ok(g & IIR_STEP_APG, {d.apg_avg, d.apg_sa, d.apg_par}))
        return IIR_EINVAL;
    if (hist_aliases(d.hist, d.x, d.prev, d.x0_out) || (d.hist && d.eps_out)) return IIR_EINVAL;
    if (d.keep_map && (d.keep_src == d.prev || d.keep_noise == d.prev)) return IIR_EINVAL;
    if (d.apg_avg && (!d.cfg || d.apg_avg == d.prev || d.apg_avg == d.x0_out || d.apg_avg == d.eps_out || d.apg_avg == d.hist))
        return IIR_EINVAL;
    return launch_1d(sched_step_kernel, (long)d.B * d.HW, stream, (const f16*)d.eps_nhwc, (long)d.lde, (int)d.B, (int)d.C, (int)d.HW,
                     (int)d.cfg, d.coef, d.pag_scale, d.x, d.noise, d.hist, d.prev, d.x0_out, d.eps_out, d.eps_factor, d.keep_map,
                     d.keep_src, d.keep_noise, d.keep_coef, d.apg_avg, d.apg_sa, d.apg_par);
}

int launch_apg_project(const void* eps_nhwc, long lde, int B, int C, int HW, const float* coef, const float* x, const float* par,
                       float* avg, float* out, void* ws, long ws_bytes, void* stream) {
    if (!eps_nhwc || !coef || !x || !par || !avg || !out || !ws || B <= 0 || C <= 0 || HW <= 0 || lde < C) return IIR_EINVAL;
    if (B > 65535 || ws_bytes < (long)B * APG_PARTS * 3 * (long)sizeof(double) || ((uintptr_t)ws & 7)) return IIR_EINVAL;
    if (avg == x || avg == out || (void*)avg == ws || (void*)out == ws) return IIR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(apg_project_kernel, dim3(APG_PARTS, B), dim3(APG_THREADS), 0, (hipStream_t)stream, (const f16*)eps_nhwc, lde, B,
                       C, HW, coef, x, par, avg, (double*)ws);
    hipLaunchKernelGGL(apg_finalize_kernel, dim3(nblk(B, 64)), dim3(64), 0, (hipStream_t)stream, (const double*)ws, B, par, out);
    return iir_launch_status();
}

}  // namespace

extern "C" int iir_sinusoid_f16(const float* vals, int32_t n_vals, int32_t rows, int32_t dim, void* out, int64_t ldo,
                                int32_t col_off, void* stream) {
    (void)hipGetLastError();
    if (!vals || !out || n_vals <= 0 || rows <= 0 || dim <= 0 || dim % 2) return IIR_EINVAL;
    const int total = rows * n_vals * (dim / 2);
    hipLaunchKernelGGL(sinusoid_kernel, dim3(nblk(total, 256)), dim3(256), 0, (hipStream_t)stream, vals, n_vals, rows, dim,
                       (f16*)out, (long)ldo, col_off);
    return iir_launch_status();
}

extern "C" int iir_silu_f16(const void* x, void* y, int64_t n, void* stream) {
    (void)hipGetLastError();
    if (!x || !y || n <= 0 || n % 8) return IIR_EINVAL;
    hipLaunchKernelGGL(silu_kernel, dim3(nblk(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const f16*)x, (f16*)y, n / 8);
    return iir_launch_status();
}

extern "C" int iir_copy_add_f16(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t dst_off, int64_t M, int32_t C,
                                const void* add, int64_t lda, const float* add_scale, int32_t rows_per_scale, void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || M <= 0 || C <= 0 || C % 8 || lds % 8 || ldd % 8 || dst_off % 8) return IIR_EINVAL;
    if (add && (lda % 8)) return IIR_EINVAL;
    if (add_scale && rows_per_scale <= 0) return IIR_EINVAL;
    hipLaunchKernelGGL(copy_add_kernel, dim3(nblk(M * (C / 8), 256)), dim3(256), 0, (hipStream_t)stream, (const f16*)src,
                       (long)lds, (f16*)dst, (long)ldd, (long)dst_off, (long)M, C, (const f16*)add, (long)lda, add_scale,
                       rows_per_scale);
    return iir_launch_status();
}

extern "C" int iir_pack_latent_t(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep,
                                 float scale, int32_t dtype, void* stream) {
    return launch_pack(x, B, C, HW, out, (long)ldo, rep, scale, nullptr, dtype, stream);
}

extern "C" int iir_pack_latent(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep,
                               float scale, void* stream) {
    return launch_pack(x, B, C, HW, out, (long)ldo, rep, scale, nullptr, IIR_DT_F16, stream);
}

extern "C" int iir_pack_latent_dscale(const float* x, int32_t B, int32_t C, int32_t HW, void* out, int64_t ldo, int32_t rep,
                                      const float* scale, int32_t dtype, void* stream) {
    if (!scale) return IIR_EINVAL;
    return launch_pack(x, B, C, HW, out, (long)ldo, rep, 1.0f, scale, dtype, stream);
}

extern "C" int iir_unpack_latent_t(const void* in, int64_t ldi, int32_t R, int32_t C, int32_t HW, float* out, int32_t dtype,
                                   void* stream) {
    return launch_unpack(in, (long)ldi, R, C, HW, out, dtype, stream);
}

extern "C" int iir_unpack_latent(const void* in, int64_t ldi, int32_t R, int32_t C, int32_t HW, float* out, void* stream) {
    return launch_unpack(in, (long)ldi, R, C, HW, out, IIR_DT_F16, stream);
}

extern "C" int iir_cfg_rescale_factor(const iir_sched_desc* d, float guidance_rescale, float* factor, void* stream) {
    return launch_cfg_rescale(d, guidance_rescale, factor, stream);
}

extern "C" int iir_sched_step(const iir_sched_desc* d, void* stream) {
    return d ? launch_sched_step(*d, stream) : IIR_EINVAL;
}

extern "C" int64_t iir_apg_project_workspace_bytes(int32_t B) {
    return B > 0 ? (int64_t)B * APG_PARTS * 3 * (int64_t)sizeof(double) : 0;
}

extern "C" int iir_apg_project(const void* eps_nhwc, int64_t lde, int32_t B, int32_t C, int32_t HW, const float* coef, const float* x,
                               const float* apg_par, float* apg_avg, float* apg_sa, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    return launch_apg_project(eps_nhwc, (long)lde, B, C, HW, coef, x, apg_par, apg_avg, apg_sa, workspace, (long)workspace_bytes, stream);
}

extern "C" int iir_copy_segments(const void* jobs, int32_t njobs, int64_t max_units, void* stream) {
    if (!jobs || njobs <= 0 || njobs > 65535 || max_units <= 0) return IIR_EINVAL;
    (void)hipGetLastError();
    const int gx = (int)(max_units < 256L * 1024 ? nblk(max_units, 256) : 1024);
    hipLaunchKernelGGL(copy_segments_kernel, dim3(gx, njobs), dim3(256), 0, (hipStream_t)stream, (const long long*)jobs);
    return iir_launch_status();
}

extern "C" int iir_lcm_step(const void* eps_nhwc, int64_t lde, int32_t B, int32_t rep, int32_t C, int32_t HW,
                            const float* coef, const float* x, void* out_nhwc, int64_t ldo, float* out_nchw, void* stream) {
    (void)hipGetLastError();
    if (!eps_nhwc || !coef || !x || !out_nhwc || B <= 0 || rep <= 0 || C <= 0 || HW <= 0 || lde < C || ldo < C) return IIR_EINVAL;
    hipLaunchKernelGGL(lcm_step_kernel, dim3(nblk((long)B * rep * HW, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)eps_nhwc, (long)lde, B, rep, C, HW, coef, x, (f16*)out_nhwc, (long)ldo, out_nchw);
    return iir_launch_status();
}

extern "C" int iir_transpose_f16(const void* in, int64_t ldi, int32_t rows, int32_t cols, void* out, int64_t ldo,
                                 int32_t rows_pad, void* stream) {
    (void)hipGetLastError();
    if (!in || !out || rows <= 0 || cols <= 0 || rows_pad < rows || ldo < rows_pad) return IIR_EINVAL;
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows_pad + 31) / 32), dim3(32, 8), 0, (hipStream_t)stream,
                       (const f16*)in, (long)ldi, rows, cols, (f16*)out, (long)ldo, rows_pad);
    return iir_launch_status();
}

// ---- per-launch timing for bench.py's roofline leg ---------------------------------------------------------------
thread_local hipEvent_t iir_armed_start = nullptr, iir_armed_stop = nullptr;

extern "C" void* iir_timing_event_create(void) {
    hipEvent_t e = nullptr;
    // timing only: no system-scope fence (an L2 write-back) when the event completes -- with it every timed launch
    // measured ~20 us longer than the same launch untimed (rocprofv3: 104.8 vs 84.8 us for the 128x160 GEMM class)
    return hipEventCreateWithFlags(&e, hipEventDisableSystemFence) == hipSuccess ? (void*)e : nullptr;
}
extern "C" void iir_timing_event_destroy(void* e) { if (e) (void)hipEventDestroy((hipEvent_t)e); }
extern "C" int iir_timing_arm(void* start, void* stop) {
    if (!start != !stop) return IIR_EINVAL;
    iir_armed_start = (hipEvent_t)start; iir_armed_stop = (hipEvent_t)stop;
    return IIR_OK;
}
extern "C" int iir_timing_elapsed_us(void* start, void* stop, float* us) {
    if (!start || !stop || !us) return IIR_EINVAL;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess) { (void)hipGetLastError(); return IIR_ELAUNCH; }
    *us = ms * 1000.f;
    return IIR_OK;
}

extern "C" int iir_abi_version(void) { return IIR_ABI_VERSION; }

namespace {
// Scheduler update on fp32 NCHW tensors (the scheduler objects' .step() API): sched_update on eps given in fp32, no guidance;
// coef = {_, sb, sa, k_x0, k_x, k_eps, k_noise, k_h}, hist optional
__global__ void sched_step_f32_kernel(const float* eps, const float* x, const float* noise, const float* coef, float* hist, long n,
                                      float* prev, float* x0_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float k[7] = {coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7]};
    sched_update(eps[i], i, k, x, noise, hist, prev, x0_out);
}
// a*x + b*y elementwise fp32 (add_noise: sqrt(abar)*x + sqrt(1-abar)*noise), coef = device {a, b}
__global__ void axpby_f32_kernel(const float* x, const float* y, const float* coef, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = axpby(coef[0], x[i], coef[1], y[i]);
}

int launch_sched_step_f32(const float* eps, const float* x, const float* noise, const float* coef, float* hist, long n, float* prev,
                          float* x0_out, void* stream) {
    if (!eps || !x || !coef || !prev || n <= 0) return IIR_EINVAL;
    if (hist_aliases(hist, x, prev, x0_out) || (hist && hist == eps)) return IIR_EINVAL;
    return launch_1d(sched_step_f32_kernel, n, stream, eps, x, noise, coef, hist, n, prev, x0_out);
}
}  // namespace

extern "C" int iir_sched_step_f32(const float* eps, const float* x, const float* noise, const float* coef, int64_t n,
                                  float* prev, float* x0_out, void* stream) {
    return launch_sched_step_f32(eps, x, noise, coef, nullptr, (long)n, prev, x0_out, stream);
}

extern "C" int iir_sched_step_hist_f32(const float* eps, const float* x, const float* noise, const float* coef, float* hist,
                                       int64_t n, float* prev, float* x0_out, void* stream) {
    if (!hist) return IIR_EINVAL;
    return launch_sched_step_f32(eps, x, noise, coef, hist, (long)n, prev, x0_out, stream);
}

extern "C" int iir_axpby_f32(const float* x, const float* y, const float* coef, int64_t n, float* out, void* stream) {
    (void)hipGetLastError();
    if (!x || !y || !coef || !out || n <= 0) return IIR_EINVAL;
    hipLaunchKernelGGL(axpby_f32_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, coef, (long)n, out);
    return iir_launch_status();
}

namespace {
// Touch one dword per 128-byte line of [p, p+bytes): pulls the range from HBM into the memory-side
// Infinity Cache (and the issuing XCD's L2) ahead of the GEMM that will stream it.
__global__ void prefetch_kernel(const char* p, long nlines) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    unsigned acc = 0;
    for (; i < nlines; i += stride) acc ^= *(const volatile unsigned*)(p + i * 128);
    asm volatile("" ::"v"(acc));
}
}  // namespace

extern "C" int iir_prefetch(const void* p, int64_t bytes, int32_t blocks, void* stream) {
    (void)hipGetLastError();
    if (!p || bytes <= 0 || blocks <= 0) return IIR_EINVAL;
    hipLaunchKernelGGL(prefetch_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const char*)p, (long)(bytes / 128));
    return iir_launch_status();
}

namespace {
// K13: seam blend of tiled VAE decode (module/diffusers_vae/autoencoder_kl.py:311-321), in place on tile b:
//   vertical:   b[.., y, x] = a[.., Ha - ext + y, x] * (1 - y/ext) + b[.., y, x] * (y/ext),  y < ext
//   horizontal: b[.., y, x] = a[.., y, Wa - ext + x] * (1 - x/ext) + b[.., y, x] * (x/ext),  x < ext
__global__ void blend_kernel(const float* a, float* b, int planes, int Ha, int Wa, int Hb, int Wb, int ext, int vertical) {
    const int rows = vertical ? ext : min(Ha, Hb), cols = vertical ? min(Wa, Wb) : ext;
    const long n = (long)planes * rows * cols;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % cols), y = (int)((i / cols) % rows), p = (int)(i / ((long)cols * rows));
    const float w = (float)(vertical ? y : x) / (float)ext;
    const float av = vertical ? a[((long)p * Ha + (Ha - ext + y)) * Wa + x] : a[((long)p * Ha + y) * Wa + (Wa - ext + x)];
    float* bp = b + ((long)p * Hb + y) * Wb + x;
    *bp = av * (1.0f - w) + *bp * w;
}
}  // namespace

extern "C" int iir_blend_tiles_f32(const float* a, float* b, int32_t planes, int32_t Ha, int32_t Wa, int32_t Hb, int32_t Wb,
                                   int32_t extent, int32_t vertical, void* stream) {
    (void)hipGetLastError();
    if (!a || !b || planes <= 0 || extent <= 0) return IIR_EINVAL;
    if (vertical ? (extent > Ha || extent > Hb) : (extent > Wa || extent > Wb)) return IIR_EINVAL;
    const long n = (long)planes * (vertical ? extent : (Ha < Hb ? Ha : Hb)) * (vertical ? (Wa < Wb ? Wa : Wb) : extent);
    hipLaunchKernelGGL(blend_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, planes, Ha, Wa, Hb, Wb, extent,
                       vertical);
    return iir_launch_status();
}
