// K1/K2/K7/K8: fp16 MFMA GEMM and implicit-GEMM convolution (NHWC) with fused epilogues, gfx950.
//
// Replaces on the reference's hot path: every nn.Linear call site of the UNet /
// Aggregator / adapters (module/ip_adapter/attention_processor.py:370,377-378,402,1140,1148-1149,
// 1173-1174,1195; GEGLU FF per module/min_sdxl.py:502-528), every 3x3 / 1x1 nn.Conv2d
// (ResnetBlock2D module/min_sdxl.py:242-283, Down/Upsample2D :598-618, SFT module/aggregator.py:70-90).
//
// Math: C[m][n] = epi( sum_k A[m][k] * W[n][k] ), fp16 operands, fp32 accumulate (MFMA 16x16x32 f16).
//   GEMM : A is [M][K] row-major (lda), W is [N][K] (torch Linear layout).
//   CONV : A row m = output pixel (img, oy, ox) of an NHWC tensor, k = (ky*ks+kx)*Cin + c; the A tile
//          is gathered straight from the input image (zero page for padding) -- no im2col buffer.
//          W is [Cout][ks][ks][Cin].  stride 1/2; `ups` folds a nearest-2x upsample into the gather.
//
// Structure: BMxBNx64 block tile, 4 waves (2x2; 8 for the 256x128 tile), operands staged by global_load_lds_dwordx4
// into an ST-deep ring of XOR-swizzled LDS images (swizzle applied on the per-lane SOURCE address so the LDS write
// stays lane-linear), fragments by ds_read_b128 double-buffered across the barrier, XCD-aware tile order.
// The weight fragment is the MFMA "A" operand so each lane ends up with 4 consecutive output columns of one row;
// the finished tile is staged through the (then idle) ring and written out in whole rows (or, for a column range,
// transposed).  Optional: LayerNorm of the A rows folded in.
#include "common.h"
#include "gemm_geo.h"
#include "../../include/instantir_hip.h"
#include <stdlib.h>
#include <type_traits>

namespace {

using iir::Geo;

constexpr int BK = 64;   // halfs per K tile = one 128-byte LDS row
// Issue-order pin (round 3).  The K loop is written as  [fragment reads of the NEXT half step] [MFMAs of the CURRENT half step],
// so that the LDS latency runs under the matrix instructions.  hipcc's scheduler sank the reads below the MFMAs and then waited
// `lgkmcnt(0)` right behind them -- one exposed LDS round trip (~200 cycles with four waves reading and the LDS-DMA writing) per
// half step, with one wave per SIMD nothing else to cover it.  A scheduling barrier after each read group keeps the source order.
#define IIR_PIN() __builtin_amdgcn_sched_barrier(0)
// The epilogue's lambdas are instantiated once per form; left to its size heuristics hipcc turns the larger ones into CALLS in the
// loader-wave builds (912 B of scratch per lane, a wave per SIMD lost, flat instead of LDS / global accesses).
#define IIR_INLINE __attribute__((always_inline))
constexpr int PF_TOUCHES = 4;   // prefetch touches per lane per launch (x 128 B x threads = up to 128-256 KiB per workgroup)

// GroupNorm-partial write-out (gn_out): 64-row slabs written side by side, and whether its LDS fits behind the staged output tile.
// One definition for the kernel, its launcher and iir_gemm_gn_supported.  The 128-row loader-wave tile writes its two slabs at
// once on 256 threads each: the thread layout of the two-per-CU 64x160 tile (id 25) it stands in for, so the partials are
// bit-identical to that tile's (the finalize kernel merges them in a fixed order).
constexpr int gn_par(int bm, bool lw) { return lw && bm == 128 ? 2 : 1; }
// LDS layout, one definition for the kernel and its launcher: the ST-deep operand ring (reused as the output tile), 256 B of
// scratch per wave (prefetch touches, dummy loads), the LayerNorm row statistics; statistics partials sit behind the output tile.
constexpr int ring_bytes(int bm, int bn, int st, bool w8) { return st * (bm * 128 + (w8 ? bn * 64 : bn * 128)); }
constexpr int scratch_bytes(int waves_m, bool lw) { return 256 * waves_m * 2 * (lw ? 2 : 1); }
constexpr int lds_bytes(int bm, int bn, int st, int waves_m, bool w8, bool lw) { return ring_bytes(bm, bn, st, w8) + scratch_bytes(waves_m, lw) + bm * 8; }
constexpr int lnp_off(int bm, int bn) { return (bm * (2 * bn + 32) + 15) / 16 * 16; }
constexpr bool ln_out_fits(int bm, int bn, int st, bool w8) { return lnp_off(bm, bn) + bm * (bn / 8) * 8 <= ring_bytes(bm, bn, st, w8); }
constexpr bool gn_out_fits(int bm, int bn, int st, int nt, bool lw, bool w8 = false) {
    const int gnt = nt / gn_par(bm, lw);
    return bm % 64 == 0 && bn <= gnt && (long)lnp_off(bm, bn) + (long)gn_par(bm, lw) * (gnt / (bn / 8)) * bn * 8 <= ring_bytes(bm, bn, st, w8);
}

// wait until at most N of this wave's vector-memory ops (the LDS-DMA loads) are outstanding, then barrier.
// One asm statement with a memory clobber: no LDS access may be scheduled across it.
template <int N>
__device__ __forceinline__ void wait_vm_lgkm_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// W8 (BASELINE configs[4]: "fp8 MFMA weights"): the weight operand is fp8-E4M3 with one fp32 scale per output channel.  Its
// tile image has 64-byte rows (64 K values), 16 rows per LDS-DMA instruction, 16-byte chunk c of row r stored at chunk
// c ^ ((r >> 2) & 3) (conflict-free 8-byte fragment reads); the activation tile stays fp16 in LDS and each A fragment is
// converted to fp8 in registers (v_cvt_scalef32_pk_fp8_f16, scale 1) -- 4 conversions per fragment, reused by all NI column
// tiles -- so the MFMA is v_mfma_f32_16x16x32_fp8_fp8.  Staged bytes per K tile drop from (BM + BN) * 128 to
// BM * 128 + BN * 64: the weight panel, which dominates the level-2 projections' fill, halves.
// LW (loader waves): the workgroup carries NW extra waves that do nothing but issue the LDS-DMA instructions of the K
// loop (and wait for them); the NW compute waves issue only fragment reads and MFMAs.  With one workgroup per CU (the
// level-2 projections: 256 tiles of 64x160) a compute wave otherwise sits ~60 cycles in the issue of every 1-KiB LDS-DMA piece,
// 7 pieces per K tile, with its SIMD's matrix pipe idle behind it (MI355X_MICROARCH.md, LDS-DMA issue cost) -- the "serial
// round trip" of DESIGN.md section 5.6.  Both kinds of wave meet at the one barrier per K tile; the protocol (tile kt+1 landed
// and tile kt's buffer drained at the barrier of iteration kt) is unchanged.  All 2*NW waves share the epilogue write-out.
// The 128x160 form (round 4, id 54) takes the 257-512-tile problems of 64x160 at one workgroup per CU: 4 loader waves issue the
// 36 pieces of a K tile (16 activation + 20 weight row groups, 9 each), 288 line requests per CU and K tile against 448 for two
// 64x160 workgroups.
// F8 (round 3): BOTH operands are fp8-E4M3 bytes.  A row of 128 K values is the same 128 bytes as a row of 64 halves, so the host
// hands the launch over with K and lda counted in 2-byte units and everything up to the fragment registers -- addresses, LDS-DMA
// staging, swizzle, conflict-free 16-byte fragment reads -- is the fp16 path unchanged; the 16 bytes a lane holds are 16 K values,
// fed to two `v_mfma_f32_16x16x32_fp8_fp8` (low and high 8 bytes: any split of the contraction index is valid as long as both
// operands use the same one).  Per K tile: the same MFMA count per K value as fp16, HALF the 128-byte lines per FLOP -- which is
// what the one-per-CU GEMMs are bound by.  Scales: wscale[n] per output channel, a_scale for the activations.
template <typename E, int BM, int BN, int ST, bool CONV, int WAVES_M = 2, bool W8 = false, bool LW = false, bool F8 = false>
__global__ __launch_bounds__(128 * WAVES_M * (LW ? 2 : 1), (WAVES_M == 2 ? 2 : 1)) void gemm_kernel(const Geo g) {
    static_assert(!(F8 && (W8 || CONV)), "the all-fp8 build covers the linear layers; W8 is the fp16-activation form");
    static_assert(!(W8 && CONV), "the fp8-weight build covers the linear layers only");
    static_assert(!(LW && W8), "loader waves: fp16 / bf16 operands only");
    static_assert(ST >= 2 && ST <= 4, "ring depths the counted waits below cover");
    using E4 = typename ET<E>::x4;
    using E8 = typename ET<E>::x8;     // (pointers stay f16-typed: both element types are 2 bytes; only conversions differ)
    constexpr int NW = WAVES_M * 2;                 // compute waves, laid out WAVES_M x 2 over the tile (= staging waves)
    constexpr int NT = 64 * NW * (LW ? 2 : 1);      // threads of the workgroup
    constexpr int WM = BM / WAVES_M, WN = BN / 2;   // wave tile
    constexpr int MI = WM / 16, NI = WN / 16;    // 16x16 MFMA tiles per wave
    constexpr int B_GROUPS = W8 ? BN / 16 : BN / 8;                   // LDS-DMA instructions that cover the weight tile
    constexpr int A_INST = BM / 8 / NW, B_INST = (B_GROUPS + NW - 1) / NW;   // glds instructions per wave per K tile
    static_assert(W8 || B_GROUPS % NW == 0, "fp16 weight tile: every wave issues the same number of row groups");
    constexpr int B_STAGE_BYTES = W8 ? BN * 64 : BN * 128;
    constexpr int RING_BYTES = ring_bytes(BM, BN, ST, W8);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16* As = (f16*)smem;                       // [ST][BM][64]
    f16* Bs = As + ST * BM * BK;                // [ST][BN][64]  (W8: [ST][BN][64 bytes])
    constexpr int LOADS = A_INST + B_INST;      // LDS-DMA instructions per wave per stage (every wave issues exactly this many)
    constexpr int SCRATCH_BYTES = scratch_bytes(WAVES_M, LW);     // 256 B per wave (prefetch touches, dummy loads)
    float2* rowstat = (float2*)(smem + RING_BYTES + SCRATCH_BYTES);          // [BM] (rstd, -rstd * mean) of this tile's rows (ln_in)
    constexpr int LNP_OFF = lnp_off(BM, BN);                                  // producer partials sit behind the finished output tile
    constexpr bool LN_OUT_FITS = ln_out_fits(BM, BN, ST, W8);
    // GroupNorm partials (round 3): per-thread column statistics of a 64-row slab meet in [row groups][BN] float2 behind the tile
    constexpr int GN_PAR = gn_par(BM, LW), GN_NT = NT / GN_PAR;              // slabs written side by side, threads per slab
    constexpr int GN_RG = GN_NT / (BN / 8);                                  // row groups of the column-fixed write-out mapping
    constexpr bool GN_OUT_FITS = gn_out_fits(BM, BN, ST, NT, LW, W8);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = LW && wave_all >= NW;                       // wave-uniform role
    const int wave = loader ? wave_all - NW : wave_all;             // index among the waves of its role
    const int wm = wave >> 1, wn = wave & 1;

    int tm, tn;
    if (!iir::tile_of_block(g, tm, tn)) return;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- per-lane staging addresses -------------------------------------------------------------
    const int srow = lane >> 3;                       // row inside an 8-row glds instruction
    const int schunk = (lane & 7) ^ srow;             // swizzled 16-byte chunk fetched by this lane
    const f16* a_src[A_INST];
    int a_pix_y[A_INST], a_pix_x[A_INST];             // conv: output pixel coords (input domain origin)
    const f16* a_img[A_INST];
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        int m = m0 + (i * NW + wave) * 8 + srow;
        if (m >= g.M) m = g.M - 1;                    // clamp: tail rows are computed and discarded
        if (!CONV) {
            a_src[i] = g.A + (long)m * g.lda + schunk * 8;
        } else {
            const int hw = g.Ho * g.Wo;
            const int img = m / hw, rem = m - img * hw;
            const int oy = rem / g.Wo, ox = rem - oy * g.Wo;
            a_img[i] = g.A + (long)img * g.x_img_stride + schunk * 8;
            a_pix_y[i] = oy * g.stride - g.pad;
            a_pix_x[i] = ox * g.stride - g.pad;
        }
    }
    const f16* b_src[B_INST];
#pragma unroll
    for (int i = 0; i < B_INST; ++i) {
        if (!W8) {
            int n = n0 + (i * NW + wave) * 8 + srow;
            if (n >= g.N) n = g.N - 1;
            b_src[i] = g.W + (long)n * g.K + schunk * 8;
        } else {                                      // 16 rows of 64 bytes per instruction; lane = (row, 16-byte chunk)
            const int r = (i * NW + wave) * 16 + (lane >> 2);
            int n = n0 + r;
            if (n >= g.N) n = g.N - 1;
            b_src[i] = (const f16*)((const char*)g.W + (long)n * g.K + (((lane & 3) ^ ((r >> 2) & 3)) * 16));
        }
    }

    // conv gather state: stage() is called for consecutive K tiles, so the (tap, channel) walk is incremental -- per tile one
    // pointer bump per row group; the pixel / padding arithmetic runs only when the tap changes (every Cin/64 tiles).  It
    // used to be redone for every tile: ~40 VALU instructions beside 40 MFMAs.
    const f16* cv_ptr[CONV ? A_INST : 1];
    int cv_inc[CONV ? A_INST : 1];
    int cv_c0 = 0, cv_tap = 0;
    auto conv_tap = [&](int tap) {
        const int ky = tap / g.ks, kx = tap - ky * g.ks;
#pragma unroll
        for (int i = 0; i < (CONV ? A_INST : 0); ++i) {
            const int iy = a_pix_y[i] + ky, ix = a_pix_x[i] + kx;
            bool ok;
            long pix;
            if (g.ups) {   // coordinates are in the 2x-upsampled domain
                ok = (iy >= 0) & (iy < 2 * g.H) & (ix >= 0) & (ix < 2 * g.Wd);
                pix = (long)(iy >> 1) * g.Wd + (ix >> 1);
            } else {
                ok = (iy >= 0) & (iy < g.H) & (ix >= 0) & (ix < g.Wd);
                pix = (long)iy * g.Wd + ix;
            }
            cv_ptr[i] = ok ? a_img[i] + pix * g.lda : g.zero + (lane & 7) * 8;      // padding pixels read the zero page, in place
            cv_inc[i] = ok ? BK : 0;
        }
    };
    auto conv_seek = [&](int kt) {
        const int k0 = kt * BK;
        cv_tap = k0 / g.Cin;
        cv_c0 = k0 - cv_tap * g.Cin;
        conv_tap(cv_tap);
#pragma unroll
        for (int i = 0; i < (CONV ? A_INST : 0); ++i) cv_ptr[i] += cv_inc[i] ? cv_c0 : 0;
    };

    auto stage = [&](int kt, int buf) {
        f16* as = As + buf * BM * BK;
        f16* bs = Bs + buf * BN * BK;
        const int k0 = kt * BK;
        if (!CONV) {
#pragma unroll
            for (int i = 0; i < A_INST; ++i) glds16(a_src[i] + k0, as + (i * NW + wave) * 8 * BK);
        } else {
#pragma unroll
            for (int i = 0; i < A_INST; ++i) {
                glds16(cv_ptr[i], as + (i * NW + wave) * 8 * BK);
                cv_ptr[i] += cv_inc[i];
            }
            cv_c0 += BK;
            if (cv_c0 == g.Cin) {
                cv_c0 = 0;
                if (++cv_tap < g.ks * g.ks) conv_tap(cv_tap);
            }
        }
        if (!W8) {
#pragma unroll
            for (int i = 0; i < B_INST; ++i) glds16(b_src[i] + k0, bs + (i * NW + wave) * 8 * BK);
        } else {
            char* bs8 = (char*)Bs + buf * B_STAGE_BYTES;
#pragma unroll
            for (int i = 0; i < B_INST; ++i) {
                if (B_GROUPS % NW == 0 || i * NW + wave < B_GROUPS) {
                    glds16((const char*)b_src[i] + k0, bs8 + (i * NW + wave) * 1024);
                } else {     // a wave without a row group this round still issues ONE vector-memory op, so the counted
                             // vmcnt waits mean the same thing in every wave: a 4-byte touch of the tile's first line
                    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)g.W, (LDS_AS void*)(smem + RING_BYTES + wave * 256), 4, 0, 0);
                }
            }
        }
    };

    // ---- fragment read offsets (bytes inside a tile image) --------------------------------------
    const int frow = lane & 15, fq = lane >> 4;
    int a_off[2], b_off[2];   // per k-step, for tile row (w*W? + i*16 + frow)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int phys = (s * 4 + fq) ^ (frow & 7);
        a_off[s] = (wm * WM + frow) * 128 + phys * 16;
        if (!W8) b_off[s] = (wn * WN + frow) * 128 + phys * 16;
        else b_off[s] = (wn * WN + frow) * 64 + ((((fq >> 1) + 2 * s) ^ ((frow >> 2) & 3)) * 16) + (fq & 1) * 8;     // (WN % 16 == 0)
    }

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- main loop: ST-deep LDS ring, tiles kt+1 .. kt+ST-2 stay in flight across the barrier ---------
    // (one barrier per K tile; the buffer refilled after the barrier is the one every wave finished
    //  reading before it arrived there)
    const int nk = g.K / BK;
    if (!LW || loader) {
        if (CONV) conv_seek(0);
#pragma unroll
        for (int s = 0; s < ST - 1; ++s)
            if (s < nk) stage(s, s);
    }
    // (Twin of iir::ln_row_stat, gemm_geo.h, which gemm8.hip calls: as a call it grows the scratch of the two 256x320 builds.)
    // LayerNorm statistics of this tile's rows: the producer's per-column-tile partials are fetched here, behind the first K
    // tiles' LDS-DMA, as ONE batch of unconditional loads, merged without a division per group and parked in LDS until the
    // epilogue.  (Measured on the 2048 x 10240 x 1280 GEGLU projection: branchy loads + Chan merges with divisions up front
    // +12.8 us; the partials held in 16 registers across the K loop and merged after it +9.4 us.)
    constexpr int MAXP = 8;
    float2 lnp_in[MAXP];
    const int ln_lt = LW ? tid - 64 * NW : tid;          // LW builds: the loader waves carry them
    if (g.ln_in && ln_lt >= 0 && ln_lt < BM) {
        const int m = min(m0 + ln_lt, g.M - 1);
#pragma unroll
        for (int j = 0; j < MAXP; ++j)              // unconditional (clamped) loads: one straight-line batch; absent groups are masked at the merge
            lnp_in[j] = ((const float2*)g.ln_in)[(long)min(j, g.ln_parts - 1) * g.M + m];

        // equal-count groups: mean = average of the group means, M2 = sum of the group M2 + cols * sum (mean_j - mean)^2
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) sm += j < g.ln_parts ? lnp_in[j].x : 0.f;
        const float inv_p = 1.0f / (float)g.ln_parts, mean = sm * inv_p;
        float m2 = 0.f, dev = 0.f;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) {
            const float d = lnp_in[j].x - mean;
            m2 += j < g.ln_parts ? lnp_in[j].y : 0.f;
            dev += j < g.ln_parts ? d * d : 0.f;
        }
        const float var = (m2 + (float)g.ln_part_cols * dev) * inv_p / (float)g.ln_part_cols;
        const float rstd = rsqrtf(var + g.ln_eps);
        rowstat[ln_lt] = make_float2(rstd, -rstd * mean);
        }

    // Software-pipelined across the barrier: the fragments of K-step 0 of tile kt+1 are fetched from LDS while the MFMAs of
    // K-step 1 of tile kt run, and the barrier that admits tile kt+1 sits between the two MFMA groups of tile kt -- so no
    // LDS-read latency is exposed after a barrier (with one workgroup per CU nothing else would hide it).  The barrier
    // also carries lgkmcnt(0): every wave's reads of tile kt are complete, so its buffer is refilled right away
    // (tile kt+ST), one tile further ahead than a refill-then-read order allows.
    using BF = std::conditional_t<W8, long, E8>;       // weight fragment: 8 fp8 bytes or 8 halves
    auto frags = [&](int buf, int s, E8 (&af)[MI], BF (&bf)[NI]) {
        const char* as = (const char*)(As + buf * BM * BK);
        const char* bs = (const char*)Bs + buf * B_STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = *(const E8*)(as + a_off[s] + i * 16 * 128);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf[j] = *(const BF*)(bs + b_off[s] + j * 16 * (W8 ? 64 : 128));
    };
    auto mma = [&](const E8 (&af)[MI], const BF (&bf)[NI]) {
        if constexpr (F8) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = iir::mfma16_f8x2(bf[j], af[i], acc[i][j]);
        } else if constexpr (!W8) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = ET<E>::mfma16(bf[j], af[i], acc[i][j]);
        } else {
            long a8[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) a8[i] = iir_fp8x8(af[i]);      // the conversion producers of fp8 operands store with
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(bf[j], a8[i], acc[i][j], 0, 0, 0);
        }
    };
    auto admit = [&](int tiles_after) {     // wait until only `tiles_after` later tiles are still in flight, all LDS reads done, barrier
        if (ST >= 4 && tiles_after >= 2) wait_vm_lgkm_and_barrier<(ST >= 4 ? 2 * LOADS : 0)>();
        else if (ST >= 3 && tiles_after >= 1) wait_vm_lgkm_and_barrier<(ST >= 3 ? LOADS : 0)>();
        else wait_vm_lgkm_and_barrier<0>();
    };
    // what the epilogue needs per column (bias, LayerNorm column sums) is requested ahead of the LAST tile's MFMAs: fetched at
    // the point of use, these loads' latency was exposed once per launch, on every wave at the same moment
    f32x4 pre_c1[NI];
    E4 pre_c0[NI];
    auto preload_cols = [&]() {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int nc = min(n0 + wn * WN + j * 16 + fq * 4, g.N - 4);       // clamped: lanes past the edge fetch a valid quad they never use
            pre_c1[j] = g.ln_in ? *(const f32x4*)(g.ln_colsum + nc) : (f32x4){0.f, 0.f, 0.f, 0.f};
            if (g.bias) pre_c0[j] = *(const E4*)((const E*)g.bias + nc);
            else for (int t = 0; t < 4; ++t) pre_c0[j][t] = (E)0.f;
        }
    };
    E8 a0[MI], a1[MI];
    BF b0[NI], b1[NI];
    // Loop form (round 3).  Per K tile the instruction order is unchanged -- [reads of half step 1][MFMAs of half step 0]
    // [barrier: next tile landed][reads of the next tile's half step 0][MFMAs of half step 1] -- but the loop now BEGINS at the
    // barrier, and the barrier's `lgkmcnt(0)` is a compiler-visible builtin.  With fragment reads pending across the back edge
    // (the first form) hipcc's wait insertion fell back to `lgkmcnt(0)` in front of every MFMA group, i.e. it also waited for the
    // reads issued one instruction earlier for the NEXT group: one exposed LDS round trip per half step.  With nothing pending at
    // the loop head the same reads get counted waits (`lgkmcnt(7)`): the prefetched group stays in flight under the MFMAs.
    auto admit2 = [&](int tiles_after) {
        __builtin_amdgcn_s_waitcnt(0xC07F);                     // lgkmcnt(0): every fragment read of the finished tile has returned
        if (ST >= 4 && tiles_after >= 2) wait_vm_and_barrier<(ST >= 4 ? 2 * LOADS : 0)>();
        else if (ST >= 3 && tiles_after >= 1) wait_vm_and_barrier<(ST >= 3 ? LOADS : 0)>();
        else wait_vm_and_barrier<0>();
    };
    if constexpr (!LW) {
        {
            const int rem = nk - 1;
            admit(rem < ST - 2 ? rem : ST - 2);
            if (ST - 1 < nk) stage(ST - 1, ST - 1);
            frags(0, 0, a0, b0);
            IIR_PIN();
            frags(0, 1, a1, b1);
            IIR_PIN();
            mma(a0, b0);
        }
        int cur = 0;
        for (int kt = 1; kt < nk; ++kt) {                 // kt = the tile this iteration admits and starts
            const int rem = nk - 1 - kt;                        // tiles that exist after kt
            admit2(rem < ST - 2 ? rem : ST - 2);
            if (kt - 1 + ST < nk) stage(kt - 1 + ST, cur);      // tile kt-1's buffer is free: every wave finished reading it
            cur = cur + 1 == ST ? 0 : cur + 1;
            frags(cur, 0, a0, b0);
            IIR_PIN();
            mma(a1, b1);                                        // tile kt-1, half step 1
            frags(cur, 1, a1, b1);
            IIR_PIN();
            mma(a0, b0);                                        // tile kt, half step 0
        }
        preload_cols();
        mma(a1, b1);
    } else if (loader) {
        // loader waves: same barriers, same counted waits, no LDS reads and no MFMAs
        {
            const int rem = nk - 1;
            admit(rem < ST - 2 ? rem : ST - 2);
            if (ST - 1 < nk) stage(ST - 1, ST - 1);
        }
        int cur = 0;
        for (int kt = 0; kt + 1 < nk; ++kt) {
            const int rem = nk - 2 - kt;
            admit(rem < ST - 2 ? rem : ST - 2);
            if (kt + ST < nk) stage(kt + ST, cur);
            cur = cur + 1 == ST ? 0 : cur + 1;
        }
    } else {
        // compute waves: they issue no vector-memory operation in the loop, so the vmcnt part of `admit` never waits
        admit(0);
        frags(0, 0, a0, b0);
        IIR_PIN();
        frags(0, 1, a1, b1);
        IIR_PIN();
        mma(a0, b0);
        int cur = 0;
        for (int kt = 1; kt < nk; ++kt) {
            admit2(0);
            cur = cur + 1 == ST ? 0 : cur + 1;
            frags(cur, 0, a0, b0);
            IIR_PIN();
            mma(a1, b1);
            frags(cur, 1, a1, b1);
            IIR_PIN();
            mma(a0, b0);
        }
        preload_cols();
        mma(a1, b1);
    }

    // ---- IIR_EPI_XATTN: `to_q` and the decoupled text / IP cross-attention of
    // TA_IPAttnProcessor2_0 (module/ip_adapter/attention_processor.py:1140-1192) in one launch.  The 64 x 128 tile is q for 64 rows
    // of one image and two heads; wave (wm, wn) holds rows 32 wm .. +32 of head wn in its accumulators.  Nothing is re-laid-out:
    // an accumulator lane (frow, fq) holds q[frow][16 j + 4 fq + t] -- as an MFMA operand that is "8 values of the contraction
    // index" for ANY consistent order of that index, so the K fragment is read in the same permuted order (two 8-byte pieces
    // per lane), S = q K^T lands as (row frow, keys 16 kb + 4 fq + t), and P feeds P V the same way with V^T read in matching
    // key order.  Both softmaxes (text keys, IP keys) are exact two-pass ones over <= 80 / 64 keys held in registers; each is
    // normalised before P V, so one accumulator sums text and IP outputs (`hidden_states + ip_hidden_states`, :1192, scale 1).
    // The K / V^T images (72 KiB: exactly the idle ring) are staged by LDS-DMA after the K loop; requesting them into registers at
    // kernel entry instead (182 VGPRs) measured SLOWER (22.3 vs 20.6 us per level-2 launch).
    bool xdone = false;
    if constexpr (BM == 64 && BN == 128 && ST == 3 && !CONV && !W8 && !LW && WAVES_M == 2 && std::is_same<E, f16>::value) {
    if (g.xa_on) {
        constexpr int KROWS = 144, KIMG = KROWS * 128, VROW = 288, VIMG = 64 * VROW;     // per head: K image 18 KiB, V^T image 18 KiB
        static_assert(2 * KIMG + 2 * VIMG <= RING_BYTES, "K / V images of two heads must fit the idle ring");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is done reading the ring
        const int img = m0 / g.xa_tq, hd0 = n0 >> 6;
        char* kl = smem;
        char* vl = smem + 2 * KIMG;
        const int tk0 = g.xa_tk[0], tk1 = g.xa_tk[1];
        const int vch0 = (tk0 + 7) >> 3, vch1 = (tk1 + 7) >> 3;               // readable 16-byte chunks of a V^T row
#pragma unroll
        for (int it = 0; it < 9; ++it) {          // K rows: [0, 80) text keys, [80, 144) IP keys; rows past Tkv repeat the last key (masked below)
            const int s = (it * 4 + wave) * 64 + lane, hh = s >= 1152 ? 1 : 0, sl = s - hh * 1152;
            const int row = sl >> 3, ch = (sl & 7) ^ (row & 7);
            const bool ip = row >= 80;
            const int key = ip ? min(row - 80, tk1 - 1) : min(row, tk0 - 1);
            const f16* src = (ip ? g.xa_k[1] + (long)img * g.xa_kb[1] + (long)key * g.xa_ldk[1]
                                 : g.xa_k[0] + (long)img * g.xa_kb[0] + (long)key * g.xa_ldk[0]) + (hd0 + hh) * 64 + ch * 8;
            glds16(src, kl + (it * 4 + wave) * 1024);
        }
#pragma unroll
        for (int it = 0; it < 9; ++it) {          // V^T rows d = 0..63 of each head: 10 chunks of text keys, 8 chunks of IP keys
            const int s = (it * 4 + wave) * 64 + lane, hh = s >= 1152 ? 1 : 0, sl = s - hh * 1152;
            const int d = sl / 18, c = sl - d * 18;
            const bool ip = c >= 10;
            const int cc = ip ? min(c - 10, vch1 - 1) : min(c, vch0 - 1);
            const long rowv = (long)((hd0 + hh) * 64 + d);
            const f16* src = (ip ? g.xa_vt[1] + rowv * g.xa_ldvt[1] + (long)img * g.xa_vb[1]
                                 : g.xa_vt[0] + rowv * g.xa_ldvt[0] + (long)img * g.xa_vb[0]) + cc * 8;
            glds16(src, vl + (it * 4 + wave) * 1024);
        }
        // q = what the plain epilogue would have stored (LayerNorm fold, bias, fp16 rounding), as MFMA operands
        typedef E E4v __attribute__((ext_vector_type(4)));
        E8 qf[MI][2];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const float2 rs = g.ln_in ? rowstat[wm * WM + i * 16 + frow] : make_float2(1.f, 0.f);
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    qf[i][j >> 1][(j & 1) * 4 + t] = (E)iir::epi_affine(acc[i][j][t], rs, pre_c1[j][t], (float)pre_c0[j][t]);
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");         // K / V images complete (waiting for K alone here and for V^T before P V measured no better)
        // S = q K^T: 9 key blocks of 16 (5 text, 4 IP), contraction over d in the accumulator's order
        f32x4 sa[MI][9];
        const char* kh = kl + wn * KIMG;
#pragma unroll
        for (int kb = 0; kb < 9; ++kb) {
            const int kr = kb * 16 + frow;
            const char* krow = kh + kr * 128 + (fq & 1) * 8;
            E8 kf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const E4v lo = *(const E4v*)(krow + (((4 * ks + (fq >> 1)) ^ (kr & 7)) << 4));
                const E4v hi = *(const E4v*)(krow + (((4 * ks + 2 + (fq >> 1)) ^ (kr & 7)) << 4));
                for (int t = 0; t < 4; ++t) { kf[ks][t] = lo[t]; kf[ks][4 + t] = hi[t]; }
            }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                z = ET<E>::mfma16(kf[0], qf[i][0], z);
                sa[i][kb] = ET<E>::mfma16(kf[1], qf[i][1], z);
            }
        }
        // softmax per segment (q carries scale x log2 e: p = exp2(s - max)), normalised, as the P operand of P V
        E8 pf[MI][5];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
            for (int kb = 0; kb < 9; ++kb)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int key = (kb < 5 ? kb * 16 : kb * 16 - 80) + fq * 4 + t;
                    const bool ok = key < (kb < 5 ? tk0 : tk1);
                    sa[i][kb][t] = ok ? sa[i][kb][t] : -INFINITY;
                    mx[kb < 5 ? 0 : 1] = fmaxf(mx[kb < 5 ? 0 : 1], sa[i][kb][t]);
                }
#pragma unroll
            for (int sgm = 0; sgm < 2; ++sgm) {
                mx[sgm] = fmaxf(mx[sgm], __shfl_xor(mx[sgm], 16, 64));
                mx[sgm] = fmaxf(mx[sgm], __shfl_xor(mx[sgm], 32, 64));
            }
            float sm[2] = {0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 9; ++kb)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float pv = __builtin_amdgcn_exp2f(sa[i][kb][t] - mx[kb < 5 ? 0 : 1]);     // masked keys: exp2(-inf) = 0
                    sa[i][kb][t] = pv;
                    sm[kb < 5 ? 0 : 1] += pv;
                }
#pragma unroll
            for (int sgm = 0; sgm < 2; ++sgm) {
                sm[sgm] += __shfl_xor(sm[sgm], 16, 64);
                sm[sgm] += __shfl_xor(sm[sgm], 32, 64);
                sm[sgm] = __builtin_amdgcn_rcpf(sm[sgm]);
            }
#pragma unroll
            for (int kp = 0; kp < 5; ++kp)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int ka = 2 * kp, kb2 = 2 * kp + 1;
                    pf[i][kp][t] = (E)(sa[i][ka][t] * sm[ka < 5 ? 0 : 1]);
                    pf[i][kp][4 + t] = kb2 < 9 ? (E)(sa[i][kb2 < 9 ? kb2 : 8][t] * sm[kb2 < 5 ? 0 : 1]) : (E)0.f;
                }
        }
        // O = P V: contraction over keys in the order P holds them (key column 16 kb + 4 fq + t: IP keys start at column 80)
        const char* vh = vl + wn * VIMG;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const char* vrow = vh + (j * 16 + frow) * VROW + fq * 8;
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kp = 0; kp < 5; ++kp) {
                const E4v lo = *(const E4v*)(vrow + (2 * kp) * 32);
                const E4v hi = *(const E4v*)(vrow + (kp < 4 ? 2 * kp + 1 : 8) * 32);       // (the ninth block's partner: P is zero there)
                E8 vf;
                for (int t = 0; t < 4; ++t) { vf[t] = lo[t]; vf[4 + t] = hi[t]; }
#pragma unroll
                for (int i = 0; i < MI; ++i) acc[i][j] = ET<E>::mfma16(vf, pf[i][kp], acc[i][j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {            // the tile now holds finished values: phase 1 adds nothing
            pre_c1[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < 4; ++t) pre_c0[j][t] = (E)0.f;
        }
        xdone = true;
    }
    }

    // ---- epilogue, phase 1: registers -> LDS.  A lane holds row m = ..+frow and 4 consecutive columns n = ..+4*fq+{0..3};
    // stored straight to memory that is 16 rows x 32 B per instruction (16 B for the paired epilogues), which made the
    // write-out -- not the K loop -- the fixed cost of every launch.  So the finished fp16 tile (bias / row bias /
    // activation / GEGLU / SFT applied) goes through the now idle ring, and phase 2 writes whole rows, 16 B per lane,
    // adding the residual from equally coalesced loads.  (fp16 rounding before the residual add = torch's own order:
    // the Linear / Conv output is an fp16 tensor before `+ residual`.)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is done reading the ring

    if (g.c_f32) {      // fp32 output straight from the accumulators (a lane holds 4 consecutive columns of one row)
        float* c32 = (float*)g.C;
        if (loader) return;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = m0 + wm * WM + i * 16 + frow;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int n = n0 + wn * WN + j * 16 + fq * 4;
                if (m < g.M && n < g.N) *(f32x4*)(c32 + (long)m * g.ldc + n) = acc[i][j] * g.out_scale;
            }
        }
        return;
    }
    const bool paired = g.epi != IIR_EPI_PLAIN;
    const int cs = (paired ? BN : 2 * BN) + 32;                          // tile row stride in bytes: odd multiple of 32 mod 256
    char* ct = smem;
    if (!loader) {
    // column-outer, row-inner: what depends on the column only (bias, fp8 scale, LayerNorm column sum) is fetched once per
    // 16-column group and lane, not once per accumulator tile (with `ln_in` the per-tile form cost the GEGLU projection 26 us)
    int lrs[MI], ms[MI];
    float2 rss[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        lrs[i] = wm * WM + i * 16 + frow;                  // row inside the tile
        ms[i] = min(m0 + lrs[i], g.M - 1);                 // tail rows: computed from clamped operands, dropped in phase 2
        rss[i] = (g.ln_in && !xdone) ? rowstat[lrs[i]] : make_float2(1.f, 0.f);
    }
    // What every form shares runs first, in place: the fp8 scales and the affine step (LayerNorm fold about the column sum, bias).
    // Columns past N read their constants at N - 4 (clamped) and are computed; phase 2 never writes them out.
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        float sc[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (W8 || F8) {
            const f32x4 ws = *(const f32x4*)(g.wscale + min(n0 + wn * WN + j * 16 + fq * 4, g.N - 4));
            for (int t = 0; t < 4; ++t) sc[t] = ws[t] * g.a_scale;
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
            for (int t = 0; t < 4; ++t)
                acc[i][j][t] = iir::epi_affine((W8 || F8) ? acc[i][j][t] * sc[t] : acc[i][j][t], rss[i], pre_c1[j][t], (float)pre_c0[j][t]);
    }
    // The rest -- plain / GEGLU / SFT, the activation, row bias or none -- is decided once, below this lambda, and is a compile-time
    // value inside it: the executed path of a launch is one straight-line block over its (j, i) quads, with no test per column group.
    // Paired columns: in every 16-column group of the (row-permuted) weight the first 8 are the "value" rows and the next 8 their
    // partners (gate for GEGLU; beta for SFT).  A lane holds 4 consecutive columns, so value lanes (fq = 0,1) and their partners
    // (fq + 2) sit 32 lanes apart: one cross-half swap per register (iir::xhalf_swap, v_permlane32_swap: VALU, no LDS round trip).
    auto phase1 = [&](auto epi_tag, auto act_tag, auto rb_tag) IIR_INLINE {
        constexpr int FORM = decltype(epi_tag)::value, ACT = decltype(act_tag)::value;
        constexpr bool RB = decltype(rb_tag)::value;
        int rb_row[RB ? MI : 1];
        long res_row[FORM == IIR_EPI_SFT ? MI : 1];
        if constexpr (RB) {
#pragma unroll
            for (int i = 0; i < MI; ++i) rb_row[i] = ms[i] / g.rows_per_rb;
        }
        if constexpr (FORM == IIR_EPI_SFT) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                long mr = ms[i];
                if (CONV && g.res_img_rows) { const int hw = g.Ho * g.Wo, img = ms[i] / hw; mr = (long)img * g.res_img_rows + (ms[i] - img * hw); }
                res_row[i] = mr;
            }
        }
        // What a column group loads at this point (row bias, the SFT `h`) is requested at its top, for all its rows at once.
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int lc = wn * WN + j * 16 + fq * 4;                   // (permuted) column held by this lane, inside the tile
            const int nl = min(n0 + lc, g.N - 4);                       // where its column constants are read
            E4 rbv[RB ? MI : 1], hv[FORM == IIR_EPI_SFT ? MI : 1];
            if constexpr (RB) {
#pragma unroll
                for (int i = 0; i < MI; ++i) rbv[i] = *(const E4*)(g.rowbias + (long)rb_row[i] * g.ldrb + nl);
            }
            if constexpr (FORM == IIR_EPI_SFT) {      // (gate lanes fetch their value lane's quad: in range, never used)
                const int col = min(n0 / 2 + (wn * WN + j * 16) / 2 + (fq & 1) * 4, g.N / 2 - 4);
#pragma unroll
                for (int i = 0; i < MI; ++i) hv[i] = *(const E4*)(g.res + res_row[i] * g.ldr + col);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int lr = lrs[i];
                float a[4];
                for (int t = 0; t < 4; ++t) a[t] = acc[i][j][t];
                if constexpr (FORM == IIR_EPI_PLAIN) {
                    if constexpr (RB) for (int t = 0; t < 4; ++t) a[t] += (float)rbv[i][t];
                    // (twin of iir::epi_act, gemm_geo.h: as a call it grows the scratch of the two 256x320 builds)
                    if constexpr (ACT == IIR_ACT_SILU) for (int t = 0; t < 4; ++t) a[t] = silu_f(a[t]);
                    else if constexpr (ACT == IIR_ACT_GELU) for (int t = 0; t < 4; ++t) a[t] = gelu_erf_f(a[t]);
                    else if constexpr (ACT == IIR_ACT_QUICKGELU) for (int t = 0; t < 4; ++t) a[t] = quick_gelu_f(a[t]);
                    E4 o;
                    for (int t = 0; t < 4; ++t) o[t] = (E)iir::rounded_f32(a[t]);
                    *(E4*)(ct + lr * cs + lc * 2) = o;
                } else if constexpr (FORM == IIR_EPI_GEGLU) {
                    // value * gelu(gate): the erf evaluation (14 VALU + v_rcp + v_exp per element) is the cost of this epilogue
                    // -- kbench 2048x10240x1280: 865 TFLOP/s plain, 735 with value lanes alone doing all four columns -- so
                    // both lanes of a pair work: the value lane finishes columns 0,1 of the quad, its gate lane columns 2,3.
                    typedef E E2 __attribute__((ext_vector_type(2)));
                    // (twin of iir::geglu_pair, gemm_geo.h, with its swap)
                    float v0, g0, v1, g1;
                    iir::xhalf_swap(a[0], a[2], v0, g0);
                    iir::xhalf_swap(a[1], a[3], v1, g1);
                    const E2 o2 = {(E)iir::rounded_f32(v0 * gelu_erf_f(g0)), (E)iir::rounded_f32(v1 * gelu_erf_f(g1))};
                    *(E2*)(ct + lr * cs + ((wn * WN + j * 16) / 2 + iir::geglu_col(fq)) * 2) = o2;
                } else {
                    // IIR_EPI_SFT: h * (gamma + 1) + beta, h from `res`; the value lanes store
                    float own, b[4];
                    for (int t = 0; t < 4; ++t) iir::xhalf_swap(a[t], a[t], own, b[t]);
                    if (fq < 2) {
                        const int lco = (wn * WN + j * 16) / 2 + fq * 4;        // output column inside the tile
                        const E4 h = hv[i];
                        E4 o;
                        for (int t = 0; t < 4; ++t) o[t] = (E)iir::rounded_f32(fmaf((float)h[t], a[t] + 1.0f, b[t]));
                        *(E4*)(ct + lr * cs + lco * 2) = o;
                    }
                }
            }
        }
    };
    using iir::form_tag;
    if (g.epi == IIR_EPI_GEGLU) phase1(form_tag<IIR_EPI_GEGLU>{}, form_tag<IIR_ACT_NONE>{}, std::false_type{});
    else if (g.epi == IIR_EPI_SFT) phase1(form_tag<IIR_EPI_SFT>{}, form_tag<IIR_ACT_NONE>{}, std::false_type{});
    else {
        auto plain = [&](auto rb_tag) IIR_INLINE {
            switch (g.act) {
                case IIR_ACT_SILU: phase1(form_tag<IIR_EPI_PLAIN>{}, form_tag<IIR_ACT_SILU>{}, rb_tag); break;
                case IIR_ACT_GELU: phase1(form_tag<IIR_EPI_PLAIN>{}, form_tag<IIR_ACT_GELU>{}, rb_tag); break;
                case IIR_ACT_QUICKGELU: phase1(form_tag<IIR_EPI_PLAIN>{}, form_tag<IIR_ACT_QUICKGELU>{}, rb_tag); break;
                default: phase1(form_tag<IIR_EPI_PLAIN>{}, form_tag<IIR_ACT_NONE>{}, rb_tag); break;
            }
        };
        if (g.rowbias) plain(std::true_type{});
        else plain(std::false_type{});
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // tile complete

    // ---- phase 2: LDS -> memory, one 16-byte chunk of a row per lane: residual loads, add, then the weight prefetch
    // for the launches that follow, then the stores.
    auto touch_next_weights = [&]() { iir::touch_next_weights<NT, PF_TOUCHES>(g, tid, smem + RING_BYTES + wave_all * 256); };
    auto write_out = [&](auto cpr_tag) {
        constexpr int CPR = decltype(cpr_tag)::value;                    // 16-byte chunks per tile row
        constexpr int TOTAL = BM * CPR, CH = (TOTAL + NT - 1) / NT;
        const int no_tile = paired ? n0 / 2 : n0, No = paired ? g.N / 2 : g.N;
        const bool use_res = g.res && !paired;
        const bool remap = CONV && (g.y_img_rows | g.res_img_rows);
        // whole tile inside the matrix, rows 16-byte addressable: straight-line code, no predicates on the loads
        const bool tr_tile = g.Ct && no_tile >= g.tr_from;                 // this whole tile lies in the transposed column range
        const bool tr_mixed = g.Ct && !tr_tile && no_tile + CPR * 8 > g.tr_from;
        const bool inside = m0 + BM <= g.M && no_tile + CPR * 8 <= No && !remap;
        const bool fast = !tr_tile && !tr_mixed && g.c_vec && (!use_res || g.r_vec) && inside;
        if (tr_tile && inside && g.ct_vec && !use_res) {
            // transposed write-out (the V third of a fused q|k|v projection becomes the V^T image the attention kernel reads):
            // a lane gathers 8 consecutive rows of one tile column from LDS and stores them as 16 contiguous bytes of Ct.
            constexpr int RC = BM / 8, TOTAL_T = (CPR * 8) * RC, CH_T = (TOTAL_T + NT - 1) / NT;
            touch_next_weights();
#pragma unroll
            for (int k = 0; k < CH_T; ++k) {
                const int idx = tid + k * NT;
                if (TOTAL_T % NT != 0 && idx >= TOTAL_T) break;
                const int c = idx / RC, rc = idx - c * RC;
                E8 o;
#pragma unroll
                for (int t = 0; t < 8; ++t) o[t] = (E)((float)*(const E*)(ct + (rc * 8 + t) * cs + c * 2) * g.out_scale);
                *(E8*)(g.Ct + (long)(no_tile + c - g.tr_from) * g.ldct + m0 + rc * 8) = o;
            }
            return;
        }
        // (hipcc drains every LDS-DMA in flight at the next use of an ordinary load's result, so the touches are issued
        //  after the residuals have been consumed and ahead of the stores, which need no wait)
        if constexpr (GN_OUT_FITS && CPR == BN / 8) {
        if (fast && g.gn_out && !paired) {
            // Write-out with GroupNorm statistics: thread = (row group rg, 16-byte column chunk cc), so
            // all rows a thread stores share its 8 channels and their sums stay in registers (taken about the thread's first
            // sample: no E[x^2] - mean^2 cancellation); per 64-row slab the RG row groups of a column are merged through LDS in
            // a fixed order by one thread per column -> (mean, M2) of the 64 stored (rounded) values of that channel.  The
            // finalize kernel merges slabs x channels of an (image, group).  No atomics: bit-reproducible.
            constexpr int RG = GN_RG, RPT = (64 + RG - 1) / RG;               // rows per thread and slab
            const int sl = GN_PAR == 1 ? 0 : tid / GN_NT, lt = tid - sl * GN_NT;    // slab group of this thread, index inside it
            const int cc = lt % CPR, rg = lt / CPR;
            const bool active = rg < RG;
            float2* part = (float2*)(smem + LNP_OFF) + sl * RG * BN;          // [GN_PAR][RG][BN]
            touch_next_weights();
#pragma unroll 1
            for (int half = sl; half < BM / 64; half += GN_PAR) {
                E8 rr[RPT];
                if (use_res) {
#pragma unroll
                    for (int j = 0; j < RPT; ++j) {
                        const int r = half * 64 + min(rg + j * RG, 63);
                        rr[j] = *(const E8*)(g.res + (long)(m0 + r) * g.ldr + no_tile + min(cc, CPR - 1) * 8);
                    }
                }
                float k0[8], s8[8], q8[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) { k0[t] = 0.f; s8[t] = 0.f; q8[t] = 0.f; }
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < RPT; ++j) {
                    const int rl = rg + j * RG;
                    if (active && rl < 64) {
                        const int r = half * 64 + rl;
                        const E8 v = *(const E8*)(ct + r * cs + cc * 16);
                        E8 o;
                        for (int t = 0; t < 8; ++t) o[t] = (E)(((float)v[t] + (use_res ? (float)rr[j][t] : 0.f)) * g.out_scale);
                        iir::store16(g.C, ((long)(m0 + r) * g.ldc + no_tile + cc * 8) * 2, o, g.st_wt != 0);
                        for (int t = 0; t < 8; ++t) {
                            const float f = (float)o[t];
                            if (j == 0) k0[t] = f;
                            const float d = f - k0[t];
                            s8[t] += d; q8[t] = fmaf(d, d, q8[t]);
                        }
                        ++cnt;
                    }
                }
                if (active) {
                    const float inv = 1.0f / (float)cnt;                      // (cnt >= 1: rg < RG <= 64)
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        part[rg * BN + cc * 8 + t] = make_float2(k0[t] + s8[t] * inv, fmaxf(q8[t] - s8[t] * s8[t] * inv, 0.f));
                }
                __syncthreads();
                if (lt < BN) {                                                // one thread per tile column: merge the row groups in order
                    float n = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll 4
                    for (int q = 0; q < RG; ++q) {
                        const float2 pq = part[q * BN + lt];
                        const float nb = (float)((64 - q + RG - 1) / RG);     // rows row group q holds in a slab
                        const float tot = n + nb, d = pq.x - mean;
                        mean += d * (nb / tot);
                        m2 += pq.y + d * d * (n * nb / tot);
                        n = tot;
                    }
                    ((float2*)g.gn_out)[(long)(m0 / 64 + half) * g.N + n0 + lt] = make_float2(mean, m2);
                }
                __syncthreads();
            }
            return;
        }
        }
        if (fast) {
            E8 o[CH];
            if (use_res) {
                E8 rr[CH];
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int c = min(tid + k * NT, TOTAL - 1), r = c / CPR, cc = c - r * CPR;
                    rr[k] = *(const E8*)(g.res + (long)(m0 + r) * g.ldr + no_tile + cc * 8);
                }
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int c = min(tid + k * NT, TOTAL - 1), r = c / CPR, cc = c - r * CPR;
                    const E8 v = *(const E8*)(ct + r * cs + cc * 16);
                    for (int t = 0; t < 8; ++t) o[k][t] = (E)(((float)v[t] + (float)rr[k][t]) * g.out_scale);
                }
            } else {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int c = min(tid + k * NT, TOTAL - 1), r = c / CPR, cc = c - r * CPR;
                    const E8 v = *(const E8*)(ct + r * cs + cc * 16);
                    for (int t = 0; t < 8; ++t) o[k][t] = (E)((float)v[t] * g.out_scale);
                }
            }
            touch_next_weights();
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int c = tid + k * NT, r = c / CPR, cc = c - r * CPR;
                if (TOTAL % NT != 0 && c >= TOTAL) break;
                if constexpr (std::is_same<E, f16>::value) {
                    if (g.c_fp8) { *(long*)((char*)g.C + (long)(m0 + r) * g.ldc + no_tile + cc * 8) = iir_fp8x8(o[k]); continue; }
                }
                iir::store16(g.C, ((long)(m0 + r) * g.ldc + no_tile + cc * 8) * 2, o[k], g.st_wt != 0);
            }
            if constexpr (LN_OUT_FITS) {
                if (g.ln_out) {
                    // the rows just written feed a LayerNorm: leave (mean, M2) of this tile's BN columns of every row, taken
                    // from the ROUNDED values (what the next GEMM reads).  Per 8-column chunk in registers, then one thread per
                    // row merges the row's CPR chunks in a fixed order (the merge weights are compile-time constants).
                    float2* lnp = (float2*)(smem + LNP_OFF);
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
                        const int c = tid + k * NT;
                        if (TOTAL % NT != 0 && c >= TOTAL) break;
                        float f[8], sum = 0.f, q = 0.f;
#pragma unroll
                        for (int t = 0; t < 8; ++t) { f[t] = (float)o[k][t]; sum += f[t]; }
                        const float mu = sum * 0.125f;
#pragma unroll
                        for (int t = 0; t < 8; ++t) { const float d = f[t] - mu; q = fmaf(d, d, q); }
                        lnp[c] = make_float2(mu, q);                                 // c = r * CPR + cc
                    }
                    __syncthreads();
                    if (tid < BM) {
                        float2 acc2 = lnp[tid * CPR];
                        float mean = acc2.x, m2 = acc2.y;
#pragma unroll
                        for (int j = 1; j < CPR; ++j) {
                            const float2 pj = lnp[tid * CPR + j];
                            const float d = pj.x - mean;
                            mean += d * (1.0f / (float)(j + 1));
                            m2 += pj.y + d * d * (8.0f * (float)j / (float)(j + 1));
                        }
                        ((float2*)g.ln_out)[(long)tn * g.M + m0 + tid] = make_float2(mean, m2);
                    }
                }
            }
        } else {
            // ragged edge / unaligned rows / per-image row remap: element-wise, speed irrelevant
            touch_next_weights();
#pragma unroll 1
            for (int c = tid; c < TOTAL; c += NT) {
                const int r = c / CPR, cc = c - r * CPR;
                const int m = m0 + r, n = no_tile + cc * 8;
                if (m >= g.M || n >= No) continue;
                long mc = m, mr = m;
                if (remap) {
                    const int hw = g.Ho * g.Wo, img = m / hw, rem = m - img * hw;
                    if (g.y_img_rows) mc = (long)img * g.y_img_rows + rem;
                    if (g.res_img_rows) mr = (long)img * g.res_img_rows + rem;
                }
                const E* tp = (const E*)(ct + r * cs + cc * 16);
#pragma unroll 1
                for (int t = 0; t < 8 && n + t < No; ++t) {
                    float v = (float)tp[t];
                    if (g.Ct && n + t >= g.tr_from) { ((E*)g.Ct)[(long)(n + t - g.tr_from) * g.ldct + mc] = (E)(v * g.out_scale); continue; }
                    if (use_res) v += (float)((const E*)g.res)[mr * g.ldr + n + t];
                    ((E*)g.C)[mc * g.ldc + n + t] = (E)(v * g.out_scale);
                }
            }
        }
    };
    if (paired) write_out(std::integral_constant<int, BN / 16>{});
    else write_out(std::integral_constant<int, BN / 8>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA touches must land before the LDS is released
}

// One kernel instantiation: tile grid, the launch-time refusals of the statistics / fp8 outputs, XCD partition, launch.
template <typename E, int BM, int BN, int ST, bool CONV, int WAVES_M = 2, bool W8 = false, bool LW = false, bool F8 = false>
int launch_k(const Geo& g0, hipStream_t stream) {
    constexpr int NT = 128 * WAVES_M * (LW ? 2 : 1);
    constexpr size_t lds = lds_bytes(BM, BN, ST, WAVES_M, W8, LW);
    Geo g = g0;
    if (g.c_fp8) {          // fp8 output: stored by the straight-line write-out only (whole tiles, 8-byte addressable rows)
        if (CONV || g.M % BM || g.N % BN || g.ldc % 8 || (uintptr_t)g.C % 8 || g.Ct || g.c_f32 || g.ln_out || g.gn_out || g.res_img_rows || g.y_img_rows ||
            (g.res && !g.r_vec) || g.dtype != IIR_DT_F16) return IIR_EINVAL;
        g.c_vec = 1; g.st_wt = 0;
    }
    if (g.gn_out) {         // producer of GroupNorm partials: whole tiles, 16-byte rows, plain epilogue, rows of an image tile-aligned (caller)
        constexpr bool fits = gn_out_fits(BM, BN, ST, NT, LW, W8);
        if (!fits || g.epi != IIR_EPI_PLAIN || g.c_f32 || g.Ct || g.ln_out || g.M % BM || g.N % BN || !g.c_vec || (g.res && !g.r_vec) ||
            (CONV && (g.y_img_rows | g.res_img_rows)))
            return IIR_EINVAL;
    }
    if (g.ln_out) {         // producer of LayerNorm partials: whole tiles, 16-byte rows, plain epilogue (see the kernel's fast write-out path)
        constexpr bool fits = ln_out_fits(BM, BN, ST, W8);
        if (!fits || CONV || g.epi != IIR_EPI_PLAIN || g.c_f32 || g.Ct || g.M % BM || g.N % BN || !g.c_vec || (g.res && !g.r_vec))
            return IIR_EINVAL;
    }
    iir::xcd_partition(g, BM, BN, 3.0 * 1048576.);      // tile grid and its XCD partition
    const dim3 grid(8 * g.rm * g.rn), block(NT);
    const auto kern = gemm_kernel<E, BM, BN, ST, CONV, WAVES_M, W8, LW, F8>;
    static unsigned long long lds_set = 0;
    if (!iir_ensure_dynamic_lds((const void*)kern, lds, lds_set)) return IIR_ELAUNCH;
    iir_launch(kern, grid, block, lds, stream, g);
    return iir_launch_status();
}

// The kernels that are built, per tile x ring depth x waves (x loader waves); anything else is refused here.
//   fp16        : GEMM and conv of every shape dispatch() names; with loader waves the conv only with the 3-deep ring
//   bf16 (VAE)  : GEMM and conv of the 4-wave two-stage tiles the chooser picks for it
//   fp8 weights (fp16 activations) and all-fp8: the linear layers on the 4-wave two-stage tiles and on 64x160x3; with loader
//                 waves the all-fp8 form of 64x160x3 only
template <int BM, int BN, int ST, int WAVES_M = 2, bool LW = false>
int launch(const Geo& g, bool conv, hipStream_t stream) {
    constexpr bool T5_3 = BM == 64 && BN == 160 && ST == 3 && WAVES_M == 2;
    constexpr bool FP8_TILE = T5_3 || (ST == 2 && WAVES_M == 2 && !LW);
    if (g.f8 || g.wscale) {
        if (conv || g.dtype != IIR_DT_F16) return IIR_EINVAL;
        if constexpr (FP8_TILE) {
            if (g.f8) return launch_k<f16, BM, BN, ST, false, WAVES_M, false, LW, true>(g, stream);
            if constexpr (!LW) return launch_k<f16, BM, BN, ST, false, WAVES_M, true>(g, stream);
        }
        return IIR_EINVAL;
    }
    if (g.dtype == IIR_DT_BF16) {
        if constexpr (ST == 2 && WAVES_M == 2 && !LW)
            return conv ? launch_k<bf16, BM, BN, ST, true>(g, stream) : launch_k<bf16, BM, BN, ST, false>(g, stream);
        return IIR_EINVAL;
    }
    if (!conv) return launch_k<f16, BM, BN, ST, false, WAVES_M, false, LW>(g, stream);
    if constexpr (!LW || ST == 3) return launch_k<f16, BM, BN, ST, true, WAVES_M, false, LW>(g, stream);
    return IIR_EINVAL;
}

struct TileShape { int bm, bn; };
constexpr TileShape kTiles[] = {{0, 0}, {128, 128}, {128, 64}, {64, 64}, {128, 160}, {64, 160}, {256, 128}};
constexpr int N_TILES = sizeof(kTiles) / sizeof(kTiles[0]) - 1;       // base shapes 1..6

// Tile choice: the per-CU operand fill rate (L2 -> LDS, ~50-70 GB/s) bounds these launches, so pick the
// shape that minimises the bytes the busiest CU has to pull.  Two workgroups per CU overlap each other's
// load latency, so capacity is counted in 512 slots: cost = ceil(blocks / 512) * 2 * (BM + BN) [* K * 2 B].
// One workgroup per CU leaves nothing else to hide the L2 -> LDS latency: launches that fit one 64x160 workgroup per CU
// (M x N = 2048 x 1280: the level-2 projections) take that tile with a 3-deep ring instead of 320 128x64 workgroups.
// Cold-weight sweep (tools/tilebench.py, us): 2048x1280x1280  128x64/2 21.9 | 64x160/3 16.7 | /4 16.3;  2048x1280x5120
// 128x64/2 67.0 | 64x160/3 47.3 | /4 46.1.  In the loop: K >= 2560 only 72.8 ms/step, K >= 1280 71.8 (3 stages), 72.7
// (4 stages) -- same call.  (With the first-generation epilogue the K = 1280 extension had measured as a loss.)
constexpr int ONE_PER_CU_MIN_K = 1280;

int pick_tile(int M, int N, bool paired, int K = 0) {
    // problems that fit one 64x160 workgroup per CU: that tile with a deep ring (see dispatch())
    if (K >= ONE_PER_CU_MIN_K && (long)((M + 63) / 64) * ((N + 159) / 160) <= 256) return 5;
    long best = -1;
    int pick = 1;
    for (int t = 1; t <= 5; ++t) {
        const long blocks = (long)((M + kTiles[t].bm - 1) / kTiles[t].bm) * ((N + kTiles[t].bn - 1) / kTiles[t].bn);
        const long cost = ((blocks + 511) / 512) * 2 * (kTiles[t].bm + kTiles[t].bn);
        if (best < 0 || cost < best || (cost == best && kTiles[t].bm * kTiles[t].bn > kTiles[pick].bm * kTiles[pick].bn)) {
            best = cost;
            pick = t;
        }
    }
    return pick;
}

// What a 4-wave-kernel launch resolves to: the dispatch() case `id` (base tile + 10 x stages, or a loader-wave build), its tile,
// ring depth and threads per workgroup.
struct Resolved { int id, bm, bn, st, nt; bool lw; };

// The one tile resolver.  Every question about what a launch will run -- dispatch() itself, iir_gemm_resolve_tile,
// iir_gemm_gn_supported, iir_gemm_ln_parts, iir_gemm_fp8_out_supported -- is answered here, so a pre-check taken while a step is
// planned and the launch it guards cannot disagree.  `tile`: 0 = automatic, 1..6 = a forced base shape (its ring depth and
// loader waves still chosen here); anything else resolves to id -1, which dispatch() refuses.  K counts 2-byte units of the
// operand row (all-fp8: the K of the fp8 bytes).  The cross-attention epilogue and the 8-wave kernel of gemm8.hip are decided
// ahead of this by dispatch().
Resolved resolve_tile(int M, int N, int K, bool conv, int dtype, bool wscale, bool f8, int tile) {
    const bool f16 = dtype == IIR_DT_F16;
    if (tile < 0 || tile > N_TILES) return {-1, 0, 0, 0, 0, false};
    if (tile == 0) {
        // problems of 257-512 64x160 tiles (M x N = 4096 x 1280, 8192 x 640) with a long K: one 128x160 loader-wave
        // workgroup per CU (id 54) instead of two 64x160 ones (id 25).  Per CU and K tile that is 288 128-byte line requests
        // against 448 for the same outputs, and these launches are paced by line requests.  fp16 activations
        // and weights only.  IIR_T4_LW=0 restores the two-per-CU choice: the bit-identity reference of the tests of id 54.
        static const bool t4_lw = !(getenv("IIR_T4_LW") && atoi(getenv("IIR_T4_LW")) == 0);
        if (t4_lw && f16 && !wscale && !f8 && K >= ONE_PER_CU_MIN_K && M % 128 == 0 && N % 160 == 0 &&
            (long)(M / 128) * (N / 160) <= 256 && (long)(M / 64) * (N / 160) > 256 && pick_tile(M, N, false, K) == 5)
            return {54, 128, 160, 3, 512, true};
        tile = pick_tile(M, N, false, K);
    }
    const int bm = kTiles[tile].bm, bn = kTiles[tile].bn;
    // ring depth: with at most one workgroup per CU nothing else hides the tile latency, and a long K loop
    // amortises the deeper prologue -> 3 stages for the 64x160 tile (measured +17..40 % on K >= 2560, M*N = 2048x1280)
    const long blocks = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    const bool one_per_cu = tile == 5 && blocks <= 256 && K >= ONE_PER_CU_MIN_K && f16;
    // one workgroup per CU: the loader-wave build, for GEMM and conv (kbench, warm: 2048x1280x1280 456 -> 535 TFLOP/s,
    // K = 5120 645 -> 707; the per-tile slope stays at the ~70 GB/s per-CU L2 -> LDS fill rate, the fixed part drops).
    // With fp8 weights it exists in the all-fp8 form only.
    if (one_per_cu && (!wscale || f8)) return {55, bm, bn, 3, 512, true};
    const int stages = one_per_cu ? 3 : 2;
    return {tile + 10 * stages, bm, bn, stages, tile == 6 ? 512 : 256, false};     // (6: the 8-wave build)
}

// Which build of the 8-wave kernel a tile = 0 launch goes to: 320 / 256 (its BN), or 0 = none (the 4-wave kernel).
//   320: the large-N linears whose 256 x 320 tiles fill the chip (the GEGLU projections);
//   256: a long-K fused q|k|v projection (transposed V range) of exactly one round of 256 x 256 tiles on at least 15/16 of the
//        CUs (240-256 tiles; the Aggregator's level-2 projection 4096 x 3840 x 1280, which the 4-wave kernel runs as 960
//        128 x 128 tiles, two per CU and twice the 128-byte line requests per FLOP).  Only that form was measured, so a plain
//        linear layer of the same shape keeps the 4-wave tile.
int gemm8_auto(const Geo& g, bool conv) {
    if (conv) return 0;
    const int K = g.f8 ? 2 * g.K : g.K;
    if (K >= 640 && (long)(g.M / 256) * (g.N / 320) >= 256 && iir::gemm8_covers(g, 320)) return 320;
    if (g.Ct && K >= 1280 && g.N % 256 == 0 && iir::gemm8_covers(g, 256)) {
        const long tiles = (long)(g.M / 256) * (g.N / 256);
        if (tiles >= 240 && tiles <= 256) return 256;
    }
    return 0;
}

int dispatch(const Geo& g, bool conv, int tile, hipStream_t stream) {
    if (g.xa_on) return conv ? IIR_EINVAL : launch<64, 128, 3>(g, false, stream);      // to_q + cross-attention: the head-aligned 64 x 128 tile, two workgroups per CU
    // tile: 0 = auto; t in {1: 128x128, 2: 128x64, 3: 64x64, 4: 128x160, 5: 64x160, 6: 256x128}; t + 10*stages selects the ring depth.
    // large-N linears whose 256 x 320 tiles fill the chip (the GEGLU projections): the 8-wave two-tile-deep kernel of
    // gemm8.hip (142 FLOP per staged byte against 71 for two 128x160 workgroups per CU).
    if (tile == 0) {
        const int bn8 = gemm8_auto(g, conv);
        if (bn8) return iir::gemm8_launch(g, bn8, stream);
    }
    if (tile == 91 || tile == 92) return conv ? IIR_EINVAL : iir::gemm8_launch(g, tile == 91 ? 320 : 256, stream);
    if (tile < 10) tile = resolve_tile(g.M, g.N, g.f8 ? 2 * g.K : g.K, conv, g.dtype, g.wscale != nullptr, g.f8 != 0, tile).id;     // (all-fp8: g.K counts 2-byte units)
    switch (tile) {
        case 21: return launch<128, 128, 2>(g, conv, stream);
        case 31: return launch<128, 128, 3>(g, conv, stream);
        case 22: return launch<128, 64, 2>(g, conv, stream);
        case 23: return launch<64, 64, 2>(g, conv, stream);
        case 24: return launch<128, 160, 2>(g, conv, stream);
        case 34: return launch<128, 160, 3>(g, conv, stream);
        case 25: return launch<64, 160, 2>(g, conv, stream);
        case 35: return launch<64, 160, 3>(g, conv, stream);
        case 54: return launch<128, 160, 3, 2, true>(g, conv, stream);    // 4 compute + 4 loader waves, one workgroup per CU
        case 55: return launch<64, 160, 3, 2, true>(g, conv, stream);
        case 65: return launch<64, 160, 4, 2, true>(g, conv, stream);
        case 75: return launch<64, 160, 2, 2, true>(g, conv, stream);     // (58 KB of LDS: two workgroups can share a CU)
        case 26: return launch<256, 128, 2, 4>(g, conv, stream);   // 8 waves, 1 workgroup per CU
        case 36: return launch<256, 128, 3, 4>(g, conv, stream);
        case 90:                                                   // 256x320, 8 waves, 72 KB per K tile: 142 FLOP per staged byte; paired
            if (g.epi == IIR_EPI_PLAIN) return IIR_EINVAL;         //   epilogues only (the half-width output tile is what fits the ring)
            return launch<256, 320, 2, 4>(g, conv, stream);
        default: return IIR_EINVAL;
    }
}

// no prefetch requested: the (unconditional) touches re-read the first line of this launch's own weights
void finish_geo(Geo& g) {
    g.st_wt = (long)g.M * g.ldc * 2 < (1L << 31);      // write-through stores (step 60.39 -> 60.22 ms); 32-bit buffer offsets
    if (g.pf_lines <= 0) { g.pf = (const char*)g.W; g.pf_lines = 1; }
    g.c_vec = (g.ldc % 8 == 0) && ((uintptr_t)g.C % 16 == 0);
    g.r_vec = g.res && (g.ldr % 8 == 0) && ((uintptr_t)g.res % 16 == 0);
}

}  // namespace

extern "C" int iir_gemm_tile_bn(int32_t tile) { tile %= 10; return (tile >= 1 && tile <= N_TILES) ? kTiles[tile].bn : -1; }

extern "C" int iir_gemm_pick_tile(int32_t M, int32_t N, int32_t K, int32_t paired) { return pick_tile(M, N, paired != 0, K); }

// Partials per row a tile = 0, plain-epilogue launch of (M, N, K) leaves in `ln_stats_out` (= N / BN of the tile it resolves to), or 0
// when that launch cannot produce them (ragged tiles).  The buffer is [parts][M] float2.
extern "C" int iir_gemm_ln_parts(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const Resolved r = resolve_tile(M, N, K, false, IIR_DT_F16, false, false, 0);
    if (M % r.bm || N % r.bn || N / r.bn > 8) return 0;      // (the consumer holds at most 8 partials per row in registers)
    return N / r.bn;
}

static int fill_gemm_geo(const iir_gemm_desc* d, Geo& g);

// 1 when the tile = 0 launch of an (M, N, K) GEMM / implicit-GEMM conv (plain epilogue, fp16) can leave GroupNorm partials
// (`gn_stats_out`): whole tiles and room for the column partials behind the staged output tile.
extern "C" int iir_gemm_gn_supported(int32_t M, int32_t N, int32_t K, int32_t is_conv) {
    if (M <= 0 || N <= 0 || K <= 0 || M % 64) return 0;
    const Resolved r = resolve_tile(M, N, K, is_conv != 0, IIR_DT_F16, false, false, 0);
    if (M % r.bm || N % r.bn) return 0;
    return gn_out_fits(r.bm, r.bn, r.st, r.nt, r.lw) ? 1 : 0;
}

// 1 when the tile = 0 all-fp8 launch of (M, N, K) can store its result as fp8 bytes (`c_fp8`): whole tiles of the tile it resolves to
extern "C" int iir_gemm_fp8_out_supported(int32_t M, int32_t N, int32_t K, int32_t paired) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 128) return 0;
    (void)paired;
    const Resolved r = resolve_tile(M, N, K, false, IIR_DT_F16, true, true, 0);
    return (M % r.bm == 0 && N % r.bn == 0) ? 1 : 0;
}

extern "C" int iir_gemm_f16(const iir_gemm_desc* d, void* stream) {
    (void)hipGetLastError();
    Geo g{};
    const int rc = fill_gemm_geo(d, g);
    if (rc != IIR_OK) return rc;
    return dispatch(g, false, d->tile, (hipStream_t)stream);
}

// Which kernel / tile `iir_gemm_f16(d)` resolves to, without launching: 91 / 92 = the 8-wave 256x320 / 256x256 kernel (gemm8.hip), 93 = the
// cross-attention tile, otherwise the dispatch() case of the 4-wave kernel (base tile + 10 x stages, or a loader-wave build such as
// 55 / 54; id % 10 is the base shape of `iir_gemm_tile_bn`), or d->tile when the caller forces one.  Used to NAME launches (bench.py roofline classes).
extern "C" int iir_gemm_resolve_tile(const iir_gemm_desc* d) {
    Geo g{};
    if (fill_gemm_geo(d, g) != IIR_OK) return -1;
    if (g.xa_on) return 93;
    if (d->tile != 0) return d->tile;
    const int bn8 = gemm8_auto(g, false);
    if (bn8) return bn8 == 320 ? 91 : 92;
    return resolve_tile(g.M, g.N, g.f8 ? 2 * g.K : g.K, false, g.dtype, g.wscale != nullptr, g.f8 != 0, 0).id;
}

static int fill_gemm_geo(const iir_gemm_desc* d, Geo& g) {
    if (!d || !d->A || !d->W || !d->C) return IIR_EINVAL;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->K % BK) return IIR_EINVAL;
    if (d->N % 4 || d->lda % 8 || d->ldc % 4) return IIR_EINVAL;
    if (d->epi != IIR_EPI_PLAIN && (d->N % 16)) return IIR_EINVAL;
    if (d->epi == IIR_EPI_SFT && !d->res) return IIR_EINVAL;
    if (d->rowbias && d->rows_per_rb <= 0) return IIR_EINVAL;
    if (d->epi < IIR_EPI_PLAIN || d->epi > IIR_EPI_XATTN) return IIR_EINVAL;
    if (d->epi == IIR_EPI_XATTN) {
        const iir_attn_kv* kv = d->xattn_kv;
        if (!kv || d->dtype != IIR_DT_F16 || d->N % 128 || d->M % 64 || d->xattn_tq <= 0 || d->xattn_tq % 64 || d->M % d->xattn_tq) return IIR_EINVAL;
        if (d->res || d->rowbias || d->act || d->Ct || d->c_f32 || d->wscale || d->ln_stats_out || d->gn_stats_out) return IIR_EINVAL;
        if (d->ldc % 8 || (uintptr_t)d->C % 16 || (d->tile != 0 && d->tile != 93)) return IIR_EINVAL;
        if (kv[0].Tkv < 1 || kv[0].Tkv > 80 || kv[1].Tkv < 1 || kv[1].Tkv > 64) return IIR_EINVAL;
        for (int sgm = 0; sgm < 2; ++sgm) {
            if (!kv[sgm].K || !kv[sgm].Vt || (uintptr_t)kv[sgm].K % 16 || (uintptr_t)kv[sgm].Vt % 16) return IIR_EINVAL;
            if (kv[sgm].ldk % 8 || kv[sgm].k_batch_stride % 8 || kv[sgm].ldvt % 8 || kv[sgm].vt_batch_stride % 8) return IIR_EINVAL;
            g.xa_k[sgm] = (const f16*)kv[sgm].K; g.xa_ldk[sgm] = kv[sgm].ldk; g.xa_kb[sgm] = kv[sgm].k_batch_stride;
            g.xa_vt[sgm] = (const f16*)kv[sgm].Vt; g.xa_ldvt[sgm] = kv[sgm].ldvt; g.xa_vb[sgm] = kv[sgm].vt_batch_stride;
            g.xa_tk[sgm] = kv[sgm].Tkv;
        }
        g.xa_on = 1; g.xa_tq = d->xattn_tq;
    }
    g.A = (const f16*)d->A; g.lda = d->lda; g.W = (const f16*)d->W; g.C = (f16*)d->C; g.ldc = d->ldc;
    g.M = d->M; g.N = d->N; g.K = d->K;
    g.bias = (const f16*)d->bias; g.rowbias = (const f16*)d->rowbias; g.ldrb = d->ldrb; g.rows_per_rb = d->rows_per_rb;
    g.res = (const f16*)d->res; g.ldr = d->ldr; g.epi = d->epi == IIR_EPI_XATTN ? IIR_EPI_PLAIN : d->epi; g.act = d->act;      // (the tile leaves the XATTN epilogue as a plain one)
    g.out_scale = d->out_scale == 0.f ? 1.f : d->out_scale;
    g.pf = (const char*)d->prefetch; g.pf_lines = d->prefetch ? (int)(d->prefetch_bytes / 128) : 0;
    finish_geo(g);
    if (d->dtype != IIR_DT_F16 && d->dtype != IIR_DT_BF16) return IIR_EINVAL;
    g.dtype = d->dtype;
    if (d->c_f32) {
        if (d->epi != IIR_EPI_PLAIN || d->bias || d->rowbias || d->res || d->Ct || d->act || d->ldc % 4 || (uintptr_t)d->C % 16) return IIR_EINVAL;
        g.c_f32 = 1;
    }
    if (d->wscale) {          // W is fp8-E4M3 [N][K] bytes with one fp32 scale per row of W
        if (d->c_f32 || d->K % 64 || (uintptr_t)d->W % 16 || (uintptr_t)d->wscale % 16 || d->dtype != IIR_DT_F16) return IIR_EINVAL;
        g.wscale = (const float*)d->wscale;
    }
    if (d->c_fp8) {
        if (d->epi == IIR_EPI_XATTN || d->epi == IIR_EPI_SFT || d->c_f32 || d->Ct || d->ln_stats_out || d->gn_stats_out || d->dtype != IIR_DT_F16) return IIR_EINVAL;
        g.c_fp8 = 1;
    }
    g.a_scale = 1.f;
    if (d->a_fp8) {           // A is fp8-E4M3 [M][K] bytes as well (lda in bytes): both operands by 128-byte rows of 128 K values
        if (!d->wscale || d->K % 128 || d->lda % 16 || (uintptr_t)d->A % 16 || d->ln_stats_in || d->epi == IIR_EPI_XATTN) return IIR_EINVAL;
        g.f8 = 1;
        g.a_scale = d->a_scale == 0.f ? 1.f : d->a_scale;
        g.K = d->K / 2; g.lda = d->lda / 2;          // counted in 2-byte units from here on: the fp16 staging path unchanged
    }
    if (d->Ct) {
        if (d->epi != IIR_EPI_PLAIN || d->tr_from < 0 || d->tr_from >= d->N || d->tr_from % 8 || d->ldct < d->M) return IIR_EINVAL;
        g.Ct = (f16*)d->Ct; g.ldct = d->ldct; g.tr_from = d->tr_from;
        g.ct_vec = (d->ldct % 8 == 0) && ((uintptr_t)d->Ct % 16 == 0);
    }
    if (d->ln_stats_out) {
        if ((uintptr_t)d->ln_stats_out % 8 || d->c_f32 || d->Ct || d->epi != IIR_EPI_PLAIN) return IIR_EINVAL;
        g.ln_out = (float*)d->ln_stats_out;
    }
    if (d->gn_stats_out) {
        if ((uintptr_t)d->gn_stats_out % 8 || d->M % 64 || d->epi != IIR_EPI_PLAIN || d->c_f32 || d->Ct || d->ln_stats_out || d->wscale) return IIR_EINVAL;
        g.gn_out = (float*)d->gn_stats_out;
    }
    if (d->ln_stats_in) {
        if (!d->ln_colsum || d->ln_parts <= 0 || d->ln_parts > 8 || d->ln_part_cols <= 0 || (long)d->ln_parts * d->ln_part_cols != d->K || d->c_f32 ||
            (uintptr_t)d->ln_stats_in % 8 || (uintptr_t)d->ln_colsum % 16 || !(d->ln_eps > 0.f)) return IIR_EINVAL;
        g.ln_in = (const float*)d->ln_stats_in; g.ln_colsum = (const float*)d->ln_colsum;
        g.ln_parts = d->ln_parts; g.ln_part_cols = d->ln_part_cols; g.ln_eps = d->ln_eps;
    }
    return IIR_OK;
}

extern "C" int iir_conv2d_nhwc_f16(const iir_conv_desc* c, void* stream) {
    (void)hipGetLastError();
    if (!c || !c->X || !c->Wt || !c->Y || !c->zero_page) return IIR_EINVAL;
    if (c->ksize != 3 && c->ksize != 1) return IIR_EINVAL;
    if (c->Cin % BK || c->ldx % 8 || c->Cout % 4 || c->ldy % 4) return IIR_EINVAL;
    if (c->stride != 1 && c->stride != 2) return IIR_EINVAL;
    if (c->upsample && c->stride != 1) return IIR_EINVAL;
    if (c->epi != IIR_EPI_PLAIN && (c->Cout % 16)) return IIR_EINVAL;
    if (c->epi == IIR_EPI_SFT && !c->res) return IIR_EINVAL;
    if (c->rowbias && c->rows_per_rb <= 0) return IIR_EINVAL;
    const int pad = c->pad_mode == 1 ? 0 : c->ksize / 2;   // mode 1: taps reach 1 pixel past the bottom/right edge only
    const int pad_hi = c->pad_mode == 1 ? 1 : pad;
    const int Hin = c->upsample ? 2 * c->H : c->H, Win = c->upsample ? 2 * c->Wd : c->Wd;
    Geo g{};
    g.Ho = (Hin + pad + pad_hi - c->ksize) / c->stride + 1;
    g.Wo = (Win + pad + pad_hi - c->ksize) / c->stride + 1;
    g.A = (const f16*)c->X; g.lda = c->ldx; g.W = (const f16*)c->Wt; g.C = (f16*)c->Y; g.ldc = c->ldy;
    g.M = c->R * g.Ho * g.Wo; g.N = c->Cout; g.K = c->ksize * c->ksize * c->Cin;
    g.bias = (const f16*)c->bias; g.rowbias = (const f16*)c->rowbias; g.ldrb = c->ldrb; g.rows_per_rb = c->rows_per_rb;
    g.res = (const f16*)c->res; g.ldr = c->ldr; g.epi = c->epi; g.act = c->act;
    g.out_scale = c->out_scale == 0.f ? 1.f : c->out_scale;
    g.H = c->H; g.Wd = c->Wd; g.Cin = c->Cin; g.ks = c->ksize; g.stride = c->stride; g.pad = pad; g.ups = c->upsample;
    g.zero = (const f16*)c->zero_page;
    g.pf = (const char*)c->prefetch; g.pf_lines = c->prefetch ? (int)(c->prefetch_bytes / 128) : 0;
    finish_geo(g);
    if (c->dtype != IIR_DT_F16 && c->dtype != IIR_DT_BF16) return IIR_EINVAL;
    g.dtype = c->dtype;
    g.x_img_stride = c->x_img_stride ? c->x_img_stride : (int64_t)c->H * c->Wd * c->ldx;
    g.y_img_rows = c->y_img_rows; g.res_img_rows = c->res_img_rows;
    if (c->gn_stats_out) {
        if ((uintptr_t)c->gn_stats_out % 8 || (g.Ho * g.Wo) % 64 || c->epi != IIR_EPI_PLAIN || c->y_img_rows || c->res_img_rows) return IIR_EINVAL;
        g.gn_out = (float*)c->gn_stats_out;
    }
    return dispatch(g, true, c->tile, (hipStream_t)stream);
}
