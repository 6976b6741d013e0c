// Separable, antialiased image resampling with PIL's filter definitions (bilinear, bicubic, Lanczos-3): the device form of
// `Image.resize` at the reference's call sites (infer.py:31-66 resize_img, infer.py:224-225, the image processors of SURVEY
// Appendix A).  Contract in include/instantir_hip.h and DESIGN.md section 7 "Resampling".  Compiled with -ffp-contract=off
// like pointwise.hip; the tap sum is written with fmaf, so it is fused by statement and nothing else is.
//
// One kernel body, one axis per launch.  The host hands over PIL's `precompute_coeffs` tables for that axis: per output
// sample a first tap, a tap count and `ksize` weights (zero padded).  A thread owns one output sample, consecutive lanes run
// along x in both passes, and the loop runs over the tap count: no compile-time tap limit, no LDS, no scratch.
//   horizontal: lane x reads its own weight row and source[row][first(x) + k]    (neighbouring lanes read neighbouring taps)
//   vertical:   a wave shares one weight row (the same y, uniform unless the row ends inside the wave) and reads
//               source[first(y) + k][x], consecutive lanes consecutive addresses
// The source is fp32 planar (N, C, H, W) or uint8 interleaved (N, H, W, C) -- an image as uploaded, 3 bytes per pixel; the
// destination is always fp32 planar and holds exactly the output window.  First tap and count are clamped into the source
// axis before use, so every load is unconditional and inside the source whatever the table holds; only the store is guarded.
// Taps are summed in index order, nothing is atomic: equal inputs give equal bits, and a windowed launch gives the bits of
// the same window cut from the full launch.
#include "image_common.h"
#include "../../include/instantir_hip.h"

namespace {

struct Pass {
    const void* src;
    float* dst;
    const int32_t* bounds;
    const float* weights;
    const float* scale;
    const float* bias;
    int C, H, W;          // source planes per image, rows, columns
    int ksize;
    int a0, b0;           // window origin along the resampled axis (output samples) and along the other axis (source samples)
    int h, w;             // destination rows, columns
    int quantize, clamp;
    float lo, hi;
};

// grid (ceil(h * w / 256), N * C), 256 threads
template <bool U8, bool VERT>
__global__ __launch_bounds__(256) void resample_pass_kernel(const Pass p) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int hw = p.h * p.w;
    const int plane = blockIdx.y;
    const int ec = min(e, hw - 1);                                   // lanes past the end recompute the last sample, unstored
    const int y = ec / p.w, x = ec - y * p.w;
    const int o = p.a0 + (VERT ? y : x);                             // output sample along the resampled axis
    const int fixed = p.b0 + (VERT ? x : y);                         // source coordinate along the other axis
    const int len = VERT ? p.H : p.W;
    const int first = min(max(p.bounds[2 * o], 0), len - 1);
    const int cnt = min(min(p.bounds[2 * o + 1], p.ksize), len - first);
    const float* wr = p.weights + (long)o * p.ksize;
    const int n = plane / p.C, c = plane - n * p.C;
    // element (row r, column q) of this plane sits at base + r * rstride + q * cstride
    const long rstride = U8 ? (long)p.W * p.C : (long)p.W;
    const long cstride = U8 ? p.C : 1;
    const long base = U8 ? (long)n * p.H * p.W * p.C + c : (long)plane * p.H * p.W;
    const long at = base + (VERT ? (long)first * rstride + (long)fixed * cstride : (long)fixed * rstride + (long)first * cstride);
    const long step = VERT ? rstride : cstride;
    float acc = 0.0f;
    if (U8) {
        const uint8_t* s = (const uint8_t*)p.src + at;
        for (int k = 0; k < cnt; ++k) acc = fmaf(wr[k], (float)s[k * step], acc);
    } else {
        const float* s = (const float*)p.src + at;
        for (int k = 0; k < cnt; ++k) acc = fmaf(wr[k], s[k * step], acc);
    }
    if (p.quantize) acc = round_u8(acc);
    if (p.clamp) acc = fminf(fmaxf(acc, p.lo), p.hi);
    if (p.scale) acc = acc * p.scale[c];
    if (p.bias) acc = acc + p.bias[c];
    if (e < hw) p.dst[(long)plane * hw + e] = acc;
}

}  // namespace

extern "C" int iir_resample_pass(const IirResampleDesc* d, void* stream) {
    if (!d || !d->src || !d->dst || !d->bounds || !d->weights) return IIR_EINVAL;
    if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->out_size <= 0 || d->ksize <= 0) return IIR_EINVAL;
    if (d->H > IIR_RESAMPLE_MAX_SIDE || d->W > IIR_RESAMPLE_MAX_SIDE || d->out_size > IIR_RESAMPLE_MAX_SIDE) return IIR_EINVAL;
    if (d->axis != 0 && d->axis != 1) return IIR_EINVAL;
    if ((int64_t)d->N * d->C > 65535) return IIR_EINVAL;                                       // grid.y
    if ((int64_t)d->out_size * d->ksize > 0x7fffffffLL) return IIR_EINVAL;
    // the window: y0 / h count rows of the destination's grid, x0 / w its columns
    const int oh = d->axis == 1 ? d->out_size : d->H, ow = d->axis == 0 ? d->out_size : d->W;
    if (d->y0 < 0 || d->x0 < 0 || d->h <= 0 || d->w <= 0) return IIR_EINVAL;
    if ((int64_t)d->y0 + d->h > oh || (int64_t)d->x0 + d->w > ow) return IIR_EINVAL;
    if ((int64_t)d->h * d->w > 0x7fffffffLL - 256) return IIR_EINVAL;
    if (d->clamp && !(d->lo <= d->hi)) return IIR_EINVAL;
    const int64_t src_bytes = (int64_t)d->N * d->C * d->H * d->W * (d->src_u8 ? 1 : (int64_t)sizeof(float));
    const int64_t dst_bytes = (int64_t)d->N * d->C * d->h * d->w * (int64_t)sizeof(float);
    if (overlap(d->src, src_bytes, d->dst, dst_bytes)) return IIR_EINVAL;
    Pass p;
    p.src = d->src; p.dst = d->dst; p.bounds = d->bounds; p.weights = d->weights; p.scale = d->scale; p.bias = d->bias;
    p.C = d->C; p.H = d->H; p.W = d->W; p.ksize = d->ksize;
    p.a0 = d->axis == 1 ? d->y0 : d->x0;
    p.b0 = d->axis == 1 ? d->x0 : d->y0;
    p.h = d->h; p.w = d->w;
    p.quantize = d->quantize; p.clamp = d->clamp; p.lo = d->lo; p.hi = d->hi;
    (void)hipGetLastError();
    const dim3 grid((unsigned)(((int64_t)d->h * d->w + 255) / 256), (unsigned)(d->N * d->C));
    hipStream_t s = (hipStream_t)stream;
    if (d->src_u8) {
        if (d->axis == 1) hipLaunchKernelGGL((resample_pass_kernel<true, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((resample_pass_kernel<true, false>), grid, dim3(256), 0, s, p);
    } else {
        if (d->axis == 1) hipLaunchKernelGGL((resample_pass_kernel<false, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((resample_pass_kernel<false, false>), grid, dim3(256), 0, s, p);
    }
    return iir_launch_status();
}
