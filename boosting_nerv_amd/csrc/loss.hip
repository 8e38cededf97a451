// loss.hip -- the high-frequency reconstruction loss of Boosting-NeRV, value AND gradient in one call.
//
// Replaces hnerv_utils.loss_fn (hnerv_utils.py:335-397) + its autograd backward, psnr_fn_single (:400-403) and the
// MS-SSIM metric (:410-412):
//     loss_b = c_l1*mean|d| + c_l2*mean d^2 + c_ms*(1 - ms_ssim_b) + c_fft*mean(|Re F(d)| + |Im F(d)|)/1 ,  d = pred - target
// (the reference takes FFT2(pred) - FFT2(target); the DFT is linear, so F(d) is the same quantity with ONE transform).
//
// Kernels (all HBM-streaming; no MFMA -- none of this is a GEMM):
//   diff_stats      sum|d|, sum d^2 per sample                                     (L1, L2, PSNR)
//   avgpool2        the MS-SSIM pyramid (2x2 mean, padding = size%2), pred and target together
//   ssim_fwd        per level: 11-tap separable Gaussian statistics in LDS -> per-tile sums of cs (levels 0-3) / ssim (4)
//   ms_coef         ms_ssim per (b,c) and d(loss)/d(level statistic)
//   ssim_bwd        per level, coarse -> fine: recompute the statistics for a haloed tile, differentiate, apply the adjoint
//                   Gaussian, add the upsampled coarser-level gradient; level 0 also adds the L1/L2 terms and writes `grad`
//   (ssim_fwd / ssim_bwd are wrappers here too: the two tile bodies -- 16-byte window loads, 4-output strips -- live in ssim_body.h)
//   (the three FFT kernels are wrappers here; plans, tables, butterflies and the row / column bodies live in fft_body.h)
//   fft_rows_fwd    in-place mixed-radix DIF FFT of every row in LDS (digit-reversed output order -- irrelevant, see below)
//   fft_cols        column DIF FFT, sum(|Re|+|Im|), S = sign(F), then the ADJOINT transform of S, all in LDS
//   fft_rows_adj    adjoint row transform, real part, accumulated into `grad`
//   ssim_head/tail  the single-scale SSIM losses (SSIM, Fusion1-6, Fusion9, L1_ssim_freq): level 0 of the above without a pyramid, as block
//                   ranges of two grids (plus three FFT launches with the spectral term) -- see "single-scale SSIM losses" below
// The forward FFT leaves its output digit-reversed; the L1 norm does not care about order and the adjoint network is the
// exact transpose-conjugate of the forward network, so no reordering pass exists anywhere.
//
// MS-SSIM follows pytorch_msssim 0.2.1 (third-party; PARITY UNPINNED).
#include "common.h"
#include "launch.h"
#include <vector>
#include <math.h>
#include <string.h>
#include <initializer_list>
#include <map>
#include <mutex>

namespace {

// =====================================================================================================================
// L1 / L2 statistics
// =====================================================================================================================
constexpr int NSB = 512;  // partial blocks per sample

__device__ __forceinline__ void diff_stats_body(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ part, int n_per_sample, const int bx, const int b) {
    const float* pp = p + (size_t)b * n_per_sample;
    const float* tt = t + (size_t)b * n_per_sample;
    float s1 = 0.f, s2 = 0.f;
    // eight loads in flight per thread; the sums take the elements in the same order as one by one
    constexpr int STR = NSB * 256;
    int i = bx * 256 + threadIdx.x;
    for (; i + 3 * STR < n_per_sample; i += 4 * STR) {
        float d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) d[u] = pp[i + u * STR] - tt[i + u * STR];
#pragma unroll
        for (int u = 0; u < 4; ++u) { s1 += fabsf(d[u]); s2 = fmaf(d[u], d[u], s2); }
    }
    for (; i < n_per_sample; i += STR) {
        const float d = pp[i] - tt[i];
        s1 += fabsf(d);
        s2 = fmaf(d, d, s2);
    }
    __shared__ float red[2][4];
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        part[((size_t)b * NSB + bx) * 2 + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    }
}
__global__ __launch_bounds__(256) void diff_stats_kernel(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ part, int n_per_sample) {
    diff_stats_body(p, t, part, n_per_sample, blockIdx.x, blockIdx.y);
}

// one wave per sample: lane-strided partial sums, then a wave reduction in fp64
__global__ __launch_bounds__(64) void psnr_final_kernel(const float* __restrict__ part, float* __restrict__ psnr, int B, int n_per_sample) {
    const int b = blockIdx.x;
    double s2 = 0.0;
    for (int k = threadIdx.x; k < NSB; k += 64) s2 += (double)part[((size_t)b * NSB + k) * 2 + 1];
    s2 = wave_sum_d(s2);
    if (threadIdx.x == 0) {
        const float mse = (float)(s2 / (double)n_per_sample);
        psnr[b] = -10.0f * log10f(mse + 1e-9f);
    }
}

// grad = k1*sign(d) + k2*d     (losses without the MS-SSIM term)
__global__ void grad_l1l2_kernel(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ g, size_t n, float k1, float k2) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float d = p[i] - t[i];
        const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
        g[i] = k1 * sg + k2 * d;
    }
}

// =====================================================================================================================
// MS-SSIM
// =====================================================================================================================
constexpr int LV = BNERV_MSSSIM_LEVELS;
constexpr int WS_ = 11, HW_ = 10;           // window size, window size - 1
constexpr int STH = 16, STW = 32;           // ssim tile
__device__ __forceinline__ int cdiv_d(int a, int b) { return (a + b - 1) / b; }

struct Win { float g[WS_]; };

struct Pyr { int H[LV], W[LV]; };

static Pyr make_pyr(int H, int W) {
    Pyr p;
    p.H[0] = H; p.W[0] = W;
    for (int l = 1; l < LV; ++l) {
        const int ph = p.H[l - 1] % 2, pw = p.W[l - 1] % 2;
        p.H[l] = (p.H[l - 1] + 2 * ph - 2) / 2 + 1;
        p.W[l] = (p.W[l - 1] + 2 * pw - 2) / 2 + 1;
    }
    return p;
}

static Win make_win() {
    // exactly pytorch_msssim._fspecial_gauss_1d in fp32: g = exp(-(x-5)^2 / (2*1.5^2)); g /= g.sum()
    Win w;
    float s = 0.f;
    for (int i = 0; i < WS_; ++i) {
        const float c = (float)(i - WS_ / 2);
        w.g[i] = expf(-(c * c) / (2.0f * 1.5f * 1.5f));
        s += w.g[i];
    }
    for (int i = 0; i < WS_; ++i) w.g[i] /= s;
    return w;
}

// 2x2 mean pool with zero padding (ph, pw), count_include_pad=True; two images per launch (blockIdx.z selects)
__global__ void avgpool2_kernel(const float* __restrict__ x0, const float* __restrict__ x1, float* __restrict__ y0, float* __restrict__ y1,
                                int planes, int H, int W, int Ho, int Wo, int ph, int pw) {
    const float* x = blockIdx.z ? x1 : x0;
    float* y = blockIdx.z ? y1 : y0;
    const size_t n = (size_t)planes * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const size_t r = i / Wo;
        const int oy = (int)(r % Ho);
        const size_t pl = r / Ho;
        const int iy = 2 * oy - ph, ix = 2 * ox - pw;
        const float* xp = x + pl * H * W;
        float s = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int yy = iy + dy, xx = ix + dx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) s += xp[(size_t)yy * W + xx];
            }
        y[i] = 0.25f * s;
    }
}

// All four coarser levels of BOTH images in one launch, for frames whose sides stay even down to level 3 (720x1280: 360, 180, 90 |
// 640, 320, 160): a block owns a 32x32 patch of level 0 = 16x16 of level 1 = ... = 2x2 of level 4, the intermediate levels pass
// through LDS.  Same arithmetic as avgpool2_kernel level by level (0.25 * (((a + b) + c) + d)), so the pyramid is bit-identical.
struct PyrArgs { const float* src[2]; float* dst[2][LV]; int H[LV], W[LV]; int planes; int vec2; };      // vec2: launcher-side flag, both sources 8-byte aligned
__device__ __forceinline__ void pyramid_body(const PyrArgs& a, const int bx, const int by, const int bz) {
    __shared__ float s1[16][17], s2[8][9], s3[4][5];
    const int img = bz & 1, pl = bz >> 1;
    const float* x = a.src[img] + (size_t)pl * a.H[0] * a.W[0];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    {
        const int oy = by * 16 + ty, ox = bx * 16 + tx;
        float v = 0.f;
        if (oy < a.H[1] && ox < a.W[1]) {
            const float* p0 = x + (size_t)(2 * oy) * a.W[0] + 2 * ox;
            const float* p1 = p0 + a.W[0];
            float2 r0, r1;
            if (a.vec2) {                                  // both images 8-byte aligned (W[0] is even here): one 8-byte load per row
                r0 = *reinterpret_cast<const float2*>(p0);
                r1 = *reinterpret_cast<const float2*>(p1);
            } else {                                       // a caller's image at an odd 4-byte boundary: the same four floats one by one
                r0 = float2{p0[0], p0[1]};
                r1 = float2{p1[0], p1[1]};
            }
            v = 0.25f * (((r0.x + r0.y) + r1.x) + r1.y);
            a.dst[img][1][((size_t)pl * a.H[1] + oy) * a.W[1] + ox] = v;
        }
        s1[ty][tx] = v;
    }
    __syncthreads();
    if (tid < 64) {
        const int y = tid >> 3, xx = tid & 7, oy = by * 8 + y, ox = bx * 8 + xx;
        const float v = 0.25f * (((s1[2 * y][2 * xx] + s1[2 * y][2 * xx + 1]) + s1[2 * y + 1][2 * xx]) + s1[2 * y + 1][2 * xx + 1]);
        if (oy < a.H[2] && ox < a.W[2]) a.dst[img][2][((size_t)pl * a.H[2] + oy) * a.W[2] + ox] = v;
        s2[y][xx] = v;
    }
    __syncthreads();
    if (tid < 16) {
        const int y = tid >> 2, xx = tid & 3, oy = by * 4 + y, ox = bx * 4 + xx;
        const float v = 0.25f * (((s2[2 * y][2 * xx] + s2[2 * y][2 * xx + 1]) + s2[2 * y + 1][2 * xx]) + s2[2 * y + 1][2 * xx + 1]);
        if (oy < a.H[3] && ox < a.W[3]) a.dst[img][3][((size_t)pl * a.H[3] + oy) * a.W[3] + ox] = v;
        s3[y][xx] = v;
    }
    __syncthreads();
    if (tid < 4) {
        const int y = tid >> 1, xx = tid & 1, oy = by * 2 + y, ox = bx * 2 + xx;
        const float v = 0.25f * (((s3[2 * y][2 * xx] + s3[2 * y][2 * xx + 1]) + s3[2 * y + 1][2 * xx]) + s3[2 * y + 1][2 * xx + 1]);
        if (oy < a.H[4] && ox < a.W[4]) a.dst[img][4][((size_t)pl * a.H[4] + oy) * a.W[4] + ox] = v;
    }
}
__global__ __launch_bounds__(256) void pyramid_kernel(const PyrArgs a) { pyramid_body(a, blockIdx.x, blockIdx.y, blockIdx.z); }

struct SsimArgs {
    const float* X; const float* Y;
    float* partial;            // fwd: [BC][tiles]
    const float* coef;         // bwd: [BC] for this level (already includes 1/Nvalid and the loss chain); NULL = coef_k for every plane
    float coef_k;              // bwd: the single-scale SSIM losses' constant chain coefficient -c_ss / (B*C*Nvalid) (the term is linear in the map)
    const float* dcoarse;      // bwd: [BC][Hc][Wc] gradient wrt the next (coarser) level's pooled image, or NULL
    float* dX;                 // bwd: [BC][H][W] written
    float* G;                  // fwd writes / bwd reads: [3][BC][H][W] UNSCALED statistic gradients (d mu1-ish, d E[xx], d E[xy]) at
                               // the valid window positions; NULL = value only.  The chain coefficient (known only after every
                               // level's forward) multiplies the backward linearly, so it is applied after the adjoint filter.
    int H, W, Hc, Wc, ph, pw;  // ph/pw: padding used when pooling THIS level into the coarser one
    int tiles_x, tiles_y;
    float C1, C2;
    float k_l1, k_l2;          // level 0 only: extra terms k_l1*sign(d) + k_l2*d
    int acc;                   // level 0 only: dX += (1) instead of dX = (0) -- the spectral gradient is already there (see loss_coarse_kernel)
    Win win;
};

// level-0 backward: the coarser levels' OWN terms (n of them), combined there; ph / pw[k]: the zero padding level k was pooled into level k + 1 with
// (0 on an even pyramid; 1080 -> 540 -> 270 -> 135 -> 68 pads 135), so pixel (y, x) of level k lies in cell ((y + ph) / 2, (x + pw) / 2)
struct CoarseChain { const float* own[LV]; int H[LV], W[LV], ph[LV], pw[LV]; int n; };

typedef float pk2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pk2 pk_fma(pk2 a, pk2 b, pk2 c) { return __builtin_elementwise_fma(a, b, c); }
#include "ssim_body.h"    // ssim_fwd_body (statistics of a tile), ssim_bwd_body (adjoint filter + chain), SSIM_BWD_LDS

// XCD-contiguous tile order of a (tiles_x, tiles_y, planes) grid: the dispatcher deals linear block ids round-robin over the 8 XCDs;
// with this remap each XCD works on a contiguous run of tiles, whose shared window rows / columns it finds in its own L2
struct Tile3 { int x, y, z; };
__device__ __forceinline__ Tile3 xcd_tile3() {
    const int gx = (int)gridDim.x, gy = (int)gridDim.y;
    const int lb = xcd_remap((int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)), (int)(gridDim.x * gridDim.y * gridDim.z));
    const int z = lb / (gx * gy), r = lb - z * (gx * gy);
    return Tile3{r % gx, r / gx, z};
}
template <bool LAST>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const SsimArgs a) { const Tile3 t = xcd_tile3(); ssim_fwd_body(a, LAST, t.x, t.y, t.z, gridDim.z); }

// every level's statistics in ONE launch (the levels only depend on the pyramid): block -> (level, tile) through the running tile counts
struct SsimAllArgs { SsimArgs lv[LV]; int first[LV + 1]; };
__global__ __launch_bounds__(256) void ssim_fwd_all_kernel(const SsimAllArgs a) {
    // neighbouring tiles share 10 of their 26 x 42 window rows / columns: each XCD (linear block ids b, b + 8, ...) takes a contiguous run of tiles
    const int lb = xcd_remap((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)(gridDim.x * gridDim.y));
    const int gbx = lb % (int)gridDim.x, gby = lb / (int)gridDim.x;
    int l = 0;
#pragma unroll
    for (int k = 1; k < LV; ++k) if (gbx >= a.first[k]) l = k;
    const int t = gbx - a.first[l];
    const int bx = t % a.lv[l].tiles_x, by = t / a.lv[l].tiles_x;
    ssim_fwd_body(a.lv[l], l == LV - 1, bx, by, gby, gridDim.y);      // (one body: its LDS arrays exist once)
}

// ---- ms_ssim per (b,c) and the chain coefficients; one block (5 waves) per (b,c) ----
struct CoefArgs {
    const float* partial[LV];   // [BC][tiles_l]
    int tiles[LV];
    float inv_nvalid[LV];
    float weights[LV];
    float* msval;               // [BC]
    float* coef;                // [LV][BC]
    int BC;
    float chain;                // -c_ms / (B*C)
};
// sum of one plane's tile partials on ONE wave: 8 loads in flight per lane (a level-0 row of 1800 partials was 29 serialised L2 round trips:
// 12 us for 3 blocks), added in fp64 in the same order as one by one, then a wave reduction; every lane returns the sum
__device__ __forceinline__ double tile_sum_d(const float* __restrict__ part, const int nt) {
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i0 = lane; i0 < nt; i0 += 8 * 64) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * 64; v[u] = i < nt ? part[i] : 0.f; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + u * 64 < nt) s += (double)v[u];
    }
    return wave_sum_d(s);
}
// one wave per level (a block of 5 waves) or, inside a 256-thread launch, waves 0..3 with wave 0 taking level 4 as well: the per-level
// sums never mix, so both forms add the same numbers in the same order
__device__ __forceinline__ void ms_coef_body(const CoefArgs& a, const int bc) {
    const int lane = threadIdx.x & 63, nw = (int)blockDim.x >> 6;
    __shared__ float stat[LV];
    for (int l = threadIdx.x >> 6; l < LV; l += nw) {
        const double s = tile_sum_d(a.partial[l] + (size_t)bc * a.tiles[l], a.tiles[l]);
        if (lane == 0) stat[l] = (float)(s * (double)a.inv_nvalid[l]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float P = 1.f;
        for (int k = 0; k < LV; ++k) P *= powf(fmaxf(stat[k], 0.f), a.weights[k]);
        a.msval[bc] = P;
        for (int k = 0; k < LV; ++k)
            a.coef[(size_t)k * a.BC + bc] = stat[k] > 0.f ? a.chain * a.weights[k] * (P / stat[k]) * a.inv_nvalid[k] : 0.f;
    }
}
__global__ __launch_bounds__(320) void ms_coef_kernel(const CoefArgs a) { ms_coef_body(a, blockIdx.x); }

template <bool LEVEL0>
__global__ __launch_bounds__(256) void ssim_bwd_from_g_kernel(const SsimArgs a) {
    __shared__ __attribute__((aligned(16))) float sl[SSIM_BWD_LDS];
    const Tile3 t = xcd_tile3(); ssim_bwd_body<LEVEL0>(a, nullptr, sl, t.x, t.y, t.z, gridDim.z);
}
__global__ __launch_bounds__(256) void ssim_bwd_level0_chain_kernel(const SsimArgs a, const CoarseChain cc) {
    __shared__ __attribute__((aligned(16))) float sl[SSIM_BWD_LDS];
    const Tile3 t = xcd_tile3(); ssim_bwd_body<true>(a, &cc, sl, t.x, t.y, t.z, gridDim.z);
}
// levels 1 .. LV-1 in one launch, each writing only its OWN term (no coarser contribution: the level-0 launch combines them)
__device__ __forceinline__ void ssim_bwd_coarse_body(const SsimAllArgs& a, float* lds, const int lin, const int gx, const int nbc) {
    const int lb = xcd_remap(lin, gx * nbc);
    const int gbx = lb % gx, gby = lb / gx;
    int l = 1;
#pragma unroll
    for (int k = 2; k < LV; ++k) if (gbx >= a.first[k]) l = k;
    const int t = gbx - a.first[l];
    const int tx = cdiv_d(a.lv[l].W, STW);
    ssim_bwd_body<false>(a.lv[l], nullptr, lds, t % tx, t / tx, gby, nbc);
}
__global__ __launch_bounds__(256) void ssim_bwd_coarse_all_kernel(const SsimAllArgs a) {
    __shared__ __attribute__((aligned(16))) float sl[SSIM_BWD_LDS];
    ssim_bwd_coarse_body(a, sl, (int)(blockIdx.x + gridDim.x * blockIdx.y), (int)gridDim.x, (int)gridDim.y);
}

#include "fft_body.h"     // the mixed-radix LDS FFT: FftPlan, make_plan, FftArgs, fft_rows_fwd_body / fft_cols_body / fft_rows_adj_body
__global__ __launch_bounds__(256) void fft_rows_fwd_kernel(const FftArgs a) { fft_rows_fwd_body(a, blockIdx.x); }
__global__ __launch_bounds__(256) void fft_cols_kernel(const FftArgs a) {      // (XCD-contiguous panels: see loss_mid_kernel)
    const int lb = xcd_remap((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)(gridDim.x * gridDim.y));
    fft_cols_body(a, lb % (int)gridDim.x, lb / (int)gridDim.x, gridDim.x);
}
__global__ __launch_bounds__(256) void fft_rows_adj_kernel(const FftArgs a) { fft_rows_adj_body(a, blockIdx.x); }

// =====================================================================================================================
// final combine: per-sample loss, batch mean, stats
// =====================================================================================================================
struct FinalArgs {
    const float* stats_part;   // [B][NSB][2]
    const float* msval;        // [BC] or NULL
    const float* fft_part;     // [BC][ncolblk] or NULL
    float* loss_out; float* stats_out;
    int B, C, n_per_sample, ncolblk;
    float c_l1, c_l2, c_ms, c_fft;
};
// one wave: lane-strided sums over the partial arrays (independent loads in flight), wave reductions in fp64
__device__ __forceinline__ void loss_final_body(const FinalArgs& a) {      // ONE wave: threadIdx.x < 64
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int b = 0; b < a.B; ++b) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = lane; k < NSB; k += 64) { s1 += (double)a.stats_part[((size_t)b * NSB + k) * 2]; s2 += (double)a.stats_part[((size_t)b * NSB + k) * 2 + 1]; }
        s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
        double l = (double)a.c_l1 * (s1 / a.n_per_sample) + (double)a.c_l2 * (s2 / a.n_per_sample);
        double ms = 0.0;
        if (a.msval) {
            for (int c = 0; c < a.C; ++c) ms += (double)a.msval[b * a.C + c];
            ms /= a.C;
            l += (double)a.c_ms * (1.0 - ms);
        }
        if (a.fft_part) {
            double f = 0.0;
            const int nf = a.C * a.ncolblk;
            for (int k = lane; k < nf; k += 64) f += (double)a.fft_part[(size_t)b * nf + k];
            f = wave_sum_d(f);
            l += (double)a.c_fft * f / (2.0 * (double)a.n_per_sample);
        }
        if (lane == 0) {
            float* so = a.stats_out + b * BNERV_LOSS_STATS;
            so[0] = (float)l; so[1] = (float)s1; so[2] = (float)s2; so[3] = (float)ms;
            // psnr_fn_single (hnerv_utils.py:400-403) on the same sums, exactly as psnr_final_kernel computes it
            const float mse = (float)(s2 / (double)a.n_per_sample);
            so[4] = -10.0f * log10f(mse + 1e-9f);
        }
        total += l;
    }
    if (lane == 0) a.loss_out[0] = (float)(total / a.B);
}
__global__ __launch_bounds__(64) void loss_final_kernel(const FinalArgs a) { loss_final_body(a); }

// ---- merged launches of the Fusion losses on an even pyramid (MS-SSIM + spectral term + gradient): the 10 launches of the branch
// sequence become 6.  What is merged are launches that do not depend on each other, as block ranges of one grid (the bodies are
// unchanged, every number is computed by the same instructions in the same order):
//   head:  row FFTs of pred - target  |  the 4-level pyramid of both images  |  the L1 / L2 partial sums
//   mid:   column FFTs (+ spectral partials, + adjoint columns)  |  the MS-SSIM coefficients (needs the SSIM launch before it)
//   tail:  level-0 SSIM gradient with the 0.25-chain  |  loss_final (needs only the partials of head and mid)
struct LossHeadArgs { FftArgs f; PyrArgs p; const float* pred; const float* target; float* stats_part; int nps, n_fft, n_pyr, pyr_gx, pyr_gy; };
__global__ __launch_bounds__(256) void loss_head_kernel(const LossHeadArgs a) {
    int b = blockIdx.x;
    if (b < a.n_fft) { fft_rows_fwd_body(a.f, b); return; }               // the long blocks first
    b -= a.n_fft;
    if (b < a.n_pyr) { const int bx = b % a.pyr_gx, r = b / a.pyr_gx; pyramid_body(a.p, bx, r % a.pyr_gy, r / a.pyr_gy); return; }
    b -= a.n_pyr;
    diff_stats_body(a.pred, a.target, a.stats_part, a.nps, b % NSB, b / NSB);
}
struct LossMidArgs { FftArgs f; CoefArgs c; int ncolblk, n_cols; };
__global__ __launch_bounds__(256) void loss_mid_kernel(const LossMidArgs a) {
    const int b = blockIdx.x;
    if (b < a.n_cols) {
        // neighbouring column panels share the 128-byte lines of every row of T: give each XCD (blocks b, b + 8, ...) a CONTIGUOUS run of
        // panels, so that a line is fetched into one L2 instead of four
        const int xcd = b & 7, k = b >> 3, per = a.n_cols >> 3, extra = a.n_cols & 7;
        const int lb = xcd * per + min(xcd, extra) + k;
        fft_cols_body(a.f, lb % a.ncolblk, lb / a.ncolblk, a.ncolblk);
    } else ms_coef_body(a.c, b - a.n_cols);
}
struct LossTailArgs { SsimArgs s; CoarseChain cc; FinalArgs fin; int gx, gy, n0, BC; };
__global__ __launch_bounds__(256) void loss_tail_kernel(const LossTailArgs a) {
    __shared__ __attribute__((aligned(16))) float sl[SSIM_BWD_LDS];
    if ((int)blockIdx.x < a.n0) { const int b = xcd_remap((int)blockIdx.x, a.n0); const int bx = b % a.gx, r = b / a.gx; ssim_bwd_body<true>(a.s, &a.cc, sl, bx, r % a.gy, r / a.gy, a.BC); }
    else if (threadIdx.x < 64) loss_final_body(a.fin);
}
// coarse:  adjoint row FFTs (the spectral gradient, WRITTEN to grad)  |  the coarser levels' SSIM gradient terms.  Both only need what `mid`
// left behind and neither fills the chip (1080 one-line blocks of 17 us, 619 short tiles at 720p); the level-0 launch then ADDS its
// gradient to the spectral one (SsimArgs::acc) instead of a sixth launch accumulating onto it.  One dynamic LDS allocation serves both bodies.
// (Slot-bound at 720p: 84 VGPRs -> 5 blocks per CU = 1280 slots for 1080 x ~14 us + 1857 x ~5.5 us of block time = 23.8 us against 12.7 + 17.9
// as two launches; forcing 80 VGPRs for a sixth block spills 22 registers in the butterflies and measured 29 us.)
struct LossCoarseArgs { FftArgs f; SsimAllArgs s; int n_adj, gx, BC; };
__global__ __launch_bounds__(256) void loss_coarse_kernel(const LossCoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x;
    if (b < a.n_adj) { fft_rows_adj_body(a.f, b); return; }              // the long blocks first
    ssim_bwd_coarse_body(a.s, sm, b - a.n_adj, a.gx, a.BC);
}
__global__ void msssim_final_kernel(const float* __restrict__ msval, float* __restrict__ out, int B, int C) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += msval[b * C + c];
    out[b] = s / C;
}

// =====================================================================================================================
// single-scale SSIM losses (hnerv_utils.py:342-361, :387-395: SSIM, Fusion1-6, Fusion9, L1_ssim_freq)
// =====================================================================================================================
// loss_b = c_l1 mean|d| + c_l2 mean d^2 + c_ss (1 - mean_c ssim_{b,c}) + c_fft (spectral term); ssim_{b,c} = mean of lum * cs over the valid
// window positions of level 0 -- ssim_fwd_body(LAST = true) and ssim_bwd_body<true> as they stand, without a pyramid.  The term is LINEAR in
// the map, so the chain coefficient is the constant SsimArgs::coef_k: no coefficient launch, and the gradient tiles wait for no reduction.
//   head:  the L1 / L2 partial sums | the statistics tiles
//   tail:  the gradient tiles (+ L1 / L2 terms, added to the spectral gradient where there is one) | the final block
// 2 launches per value + gradient call; 5 with the spectral term (row FFTs, head, column FFTs, adjoint row FFTs writing `grad`, tail).

// ssim_{b,c} of one plane from its tile partials: ONE wave (tile_sum_d, the reduction of ms_coef_body)
__device__ __forceinline__ void ssim_plane_body(const float* __restrict__ part, const int nt, const float inv_nvalid, float* val, const int bc) {
    const double s = tile_sum_d(part + (size_t)bc * nt, nt);
    if ((threadIdx.x & 63) == 0) val[bc] = (float)(s * (double)inv_nvalid);
}
struct SsimFinalArgs { const float* part; float* val; float inv_nvalid; int tiles, BC; FinalArgs fin; };
// every plane's value, the planes over the block's waves; the block may read a.val afterwards
__device__ __forceinline__ void ssim_planes_body(const SsimFinalArgs& a) {
    const int nw = (int)blockDim.x >> 6;
    for (int bc = threadIdx.x >> 6; bc < a.BC; bc += nw) ssim_plane_body(a.part, a.tiles, a.inv_nvalid, a.val, bc);
    __threadfence();
    __syncthreads();
}
// ... then loss_final_body on wave 0 with (msval, c_ms) = (the planes' SSIM, c_ss): the same combine
__device__ __forceinline__ void ssim_final_body(const SsimFinalArgs& a) {
    ssim_planes_body(a);
    if (threadIdx.x < 64) loss_final_body(a.fin);
}
__global__ __launch_bounds__(256) void ssim_final_kernel(const SsimFinalArgs a) { ssim_final_body(a); }

// The spectral term of this path holds its own instantiations of the FFT bodies with generic-radix arrays of SSIM_FFT_MAX_RADIX entries: an
// 11 x 37 frame is a legal size here (no min(H, W) > 160), and 37 is prime.  The kernels of bnerv_loss_fwd_bwd keep BNERV_FFT_MAX_RADIX.
constexpr int SSIM_FFT_MAX_RADIX = 37;
__global__ __launch_bounds__(256) void ssim_fft_cols_kernel(const FftArgs a) {
    const int lb = xcd_remap((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)(gridDim.x * gridDim.y));
    fft_cols_body<SSIM_FFT_MAX_RADIX>(a, lb % (int)gridDim.x, lb / (int)gridDim.x, gridDim.x);
}
__global__ __launch_bounds__(256) void ssim_fft_rows_fwd_kernel(const FftArgs a) { fft_rows_fwd_body<SSIM_FFT_MAX_RADIX>(a, blockIdx.x); }
__global__ __launch_bounds__(256) void ssim_fft_rows_adj_kernel(const FftArgs a) { fft_rows_adj_body<SSIM_FFT_MAX_RADIX>(a, blockIdx.x); }

// [L1 / L2 partial sums | level-0 statistics tiles].  The row FFTs of the spectral term are NOT a block range of this grid (as they are in
// loss_head_kernel): their dynamic LDS (25.6 KB at W = 1280) next to the tiles' 22 KB leaves 3 blocks per CU, and the merged kernel measured
// 5 % (720p) to 16 % (1080p) of the whole call slower than the row FFTs in a launch of their own (profiles/ssim_loss.md).
struct SsimHeadArgs { SsimArgs s; const float* pred; const float* target; float* stats_part; int nps, n_sums, BC; };
__global__ __launch_bounds__(256) void ssim_head_kernel(const SsimHeadArgs a) {
    int b = blockIdx.x;
    if (b < a.n_sums) { diff_stats_body(a.pred, a.target, a.stats_part, a.nps, b % NSB, b / NSB); return; }   // (NSB is a multiple of 8)
    b -= a.n_sums;
    const int nt = a.s.tiles_x * a.s.tiles_y;
    const int t = xcd_remap(b, nt * a.BC);
    const int bc = t / nt, r = t - bc * nt;
    ssim_fwd_body(a.s, true, r % a.s.tiles_x, r / a.s.tiles_x, bc, a.BC);
}

struct SsimTailArgs { SsimArgs s; SsimFinalArgs fin; int gx, gy, n0, BC; };
__global__ __launch_bounds__(256) void ssim_tail_kernel(const SsimTailArgs a) {
    __shared__ __attribute__((aligned(16))) float sl[SSIM_BWD_LDS];
    if ((int)blockIdx.x < a.n0) { const int b = xcd_remap((int)blockIdx.x, a.n0); const int bx = b % a.gx, r = b / a.gx; ssim_bwd_body<true>(a.s, nullptr, sl, bx, r % a.gy, r / a.gy, a.BC); }
    else ssim_final_body(a.fin);
}
// the metric: out[b] = mean_c ssim_{b,c}, the same sums as stats_out column 3 of the loss (loss_final_body)
__global__ __launch_bounds__(256) void ssim_metric_kernel(const SsimFinalArgs a, float* __restrict__ out, int B, int C) {
    ssim_planes_body(a);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        double ms = 0.0;
        for (int c = 0; c < C; ++c) ms += (double)a.val[b * C + c];
        ms /= C;
        out[b] = (float)ms;
    }
}

// =====================================================================================================================
// workspace layout
// =====================================================================================================================
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;
constexpr float MS_WEIGHTS[LV] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};

struct WsLayout {
    size_t stats_part, pyrX[LV], pyrY[LV], dXl[LV], Gl[LV], ssim_part[LV], msval, coef, T, fft_part, total;
    int tiles_x[LV], tiles_y[LV], tiles[LV];          // statistics tiles of a level: its valid window positions in STH x STW tiles
    Pyr pyr;
    int ncolblk, BC;
};
static size_t align64(size_t x) { return (x + 63) & ~size_t(63); }
// levels: LV = MS-SSIM; 1 = the single-scale SSIM losses (level 0 only: three statistic-gradient maps, tile partials and the planes' values, no
// pooled images, no coefficient array); 0 = the L1 / L2 partial sums alone (bnerv_psnr)
static WsLayout make_layout(int B, int C, int H, int W, int levels, bool use_fft) {
    WsLayout L{};
    size_t off = 0;                                   // in floats
    auto take = [&](size_t n) { size_t o = off; off = align64(off + n); return o; };
    const size_t BC = (size_t)B * C;
    L.BC = (int)BC;
    L.stats_part = take((size_t)B * NSB * 2);
    if (levels) L.pyr = make_pyr(H, W);
    for (int l = 0; l < levels; ++l) {
        const size_t n = BC * L.pyr.H[l] * L.pyr.W[l];
        if (l > 0) { L.pyrX[l] = take(n); L.pyrY[l] = take(n); L.dXl[l] = take(n); }
        L.Gl[l] = take(3 * n);
        L.tiles_x[l] = cdiv(L.pyr.W[l] - HW_, STW); L.tiles_y[l] = cdiv(L.pyr.H[l] - HW_, STH); L.tiles[l] = L.tiles_y[l] * L.tiles_x[l];
        L.ssim_part[l] = take(BC * L.tiles[l]);
    }
    if (levels) L.msval = take(BC);
    if (levels == LV) L.coef = take(BC * LV);
    if (use_fft) {
        L.ncolblk = cdiv(W / 2 + 1, COLS_PER_BLOCK);
        L.T = take(BC * H * (size_t)(W / 2 + 1) * 2);
        L.fft_part = take(BC * L.ncolblk);
    }
    L.total = off;
    return L;
}

// =====================================================================================================================
// kernel arguments: one builder per struct
// =====================================================================================================================
// SsimArgs of level l of (X, Y): what the layout decides, for both passes.  A site overrides only what is its own: G = NULL (value only: the
// statistic-gradient maps are not written), coef = NULL + coef_k (single scale), k_l1 / k_l2 / acc (level 0 of a backward), and dcoarse / Hc / Wc /
// ph / pw in the level-by-level backward ALONE -- ssim_bwd_body reads them whenever dcoarse is set; the fused forms carry the chain in CoarseChain.
static SsimArgs level_args(const float* X, const float* Y, float* grad, float* ws, const WsLayout& L, int l) {
    static const Win win = make_win();
    SsimArgs a{};
    a.X = l ? ws + L.pyrX[l] : X; a.Y = l ? ws + L.pyrY[l] : Y; a.dX = l ? ws + L.dXl[l] : grad; a.G = ws + L.Gl[l];
    a.partial = ws + L.ssim_part[l]; a.coef = ws + L.coef + (size_t)l * L.BC;
    a.H = L.pyr.H[l]; a.W = L.pyr.W[l]; a.tiles_x = L.tiles_x[l]; a.tiles_y = L.tiles_y[l];
    a.C1 = SSIM_C1; a.C2 = SSIM_C2; a.win = win;
    return a;
}
static float inv_nvalid(const WsLayout& L, int l) { return 1.0f / ((float)(L.pyr.H[l] - HW_) * (float)(L.pyr.W[l] - HW_)); }

static CoefArgs coef_args(float* ws, const WsLayout& L, float chain) {
    CoefArgs ca{};
    for (int l = 0; l < LV; ++l) { ca.partial[l] = ws + L.ssim_part[l]; ca.tiles[l] = L.tiles[l]; ca.inv_nvalid[l] = inv_nvalid(L, l); ca.weights[l] = MS_WEIGHTS[l]; }
    ca.msval = ws + L.msval; ca.coef = ws + L.coef; ca.BC = L.BC; ca.chain = chain;
    return ca;
}
// the pyramid and every level's statistics (one launch or one per level), of an even or an odd pyramid
static int ms_forward_args(const float* X, const float* Y, float* ws, const WsLayout& L, bool want_g, PyrArgs& pa, SsimAllArgs& sa) {
    pa.src[0] = X; pa.src[1] = Y; pa.planes = L.BC;
    pa.vec2 = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 7) == 0 ? 1 : 0;
    int nblk = 0;
    for (int l = 0; l < LV; ++l) {
        pa.H[l] = L.pyr.H[l]; pa.W[l] = L.pyr.W[l];
        if (L.pyr.H[l] <= HW_ || L.pyr.W[l] <= HW_) return bnerv_set_error(BNERV_E_ARG, "ms_ssim: level %d is %dx%d, needs > %d on both sides", l, L.pyr.H[l], L.pyr.W[l], HW_);
        if (l > 0) { pa.dst[0][l] = ws + L.pyrX[l]; pa.dst[1][l] = ws + L.pyrY[l]; }
        sa.lv[l] = level_args(X, Y, nullptr, ws, L, l);
        if (!want_g) sa.lv[l].G = nullptr;
        sa.first[l] = nblk;
        nblk += L.tiles[l];
    }
    sa.first[LV] = nblk;
    return BNERV_OK;
}
// the fused backward launches (the coarser levels' own terms; level 0 with the 0.25-chain over them), of an even or an odd pyramid
static void ms_backward_args(const float* X, const float* Y, float* grad, float* ws, const WsLayout& L, float k_l1, float k_l2, int acc, SsimAllArgs& sa, CoarseChain& cc) {
    int nblk = 0;
    for (int l = 0; l < LV; ++l) {
        const SsimArgs& a = sa.lv[l] = level_args(X, Y, grad, ws, L, l);
        sa.first[l] = nblk;
        if (l >= 1) nblk += cdiv(a.W, STW) * cdiv(a.H, STH);
        cc.own[l] = l ? a.dX : nullptr; cc.H[l] = a.H; cc.W[l] = a.W; cc.ph[l] = a.H % 2; cc.pw[l] = a.W % 2;
    }
    sa.lv[0].k_l1 = k_l1; sa.lv[0].k_l2 = k_l2; sa.lv[0].acc = acc;
    sa.first[LV] = nblk;
    cc.n = LV - 1;
}

// a checked descriptor and what both *_fwd_bwd entry points derive from it; `who` prefixes the messages
struct LossCall { bnerv_loss_desc d; int nps, BC; float k_l1, k_l2; };
static int open_loss_call(const bnerv_loss_desc* dp, const char* who, LossCall& c) {
    BNERV_REQUIRE(dp != nullptr, "%s: null descriptor", who);
    const bnerv_loss_desc& d = c.d = *dp;
    BNERV_REQUIRE(d.pred && d.target && d.loss_out && d.stats_out && d.ws, "%s: null tensor", who);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(d.ws) & 7) == 0, "%s: ws must be 8-byte aligned (the spectral term keeps its float2 spectra in it)", who);
    BNERV_REQUIRE(d.B > 0 && d.C > 0 && d.H > 0 && d.W > 0 && d.B <= 65535, "%s: bad dims", who);
    BNERV_REQUIRE((size_t)d.C * d.H * d.W < (size_t)1 << 31, "%s: sample too large", who);
    c.nps = d.C * d.H * d.W; c.BC = d.B * d.C;
    c.k_l1 = d.c_l1 / ((float)d.B * (float)c.nps); c.k_l2 = 2.0f * d.c_l2 / ((float)d.B * (float)c.nps);
    return BNERV_OK;
}
// Static LDS of the kernels that carry an FFT body, which a block needs ON TOP of the dynamic bytes of its lines and tables: the row bodies declare
// none, fft_cols_body its 16-byte reduction, and a merged kernel whatever its other bodies declare (loss_head: the pyramid tile and the L1 / L2 sums).
// Read from the loaded code object, once per entry point: `row` / `col` = the largest of the kernels that may run the row / column bodies there.
constexpr size_t FFT_LDS_PER_BLOCK = 160 * 1024;
struct FftStaticLds { size_t row = 0, col = 0; bool known = false; };
static bool fft_static_lds(std::initializer_list<const void*> rows, std::initializer_list<const void*> cols, FftStaticLds& out) {
    static std::mutex m;
    std::lock_guard<std::mutex> lk(m);
    if (out.known) return true;
    FftStaticLds s;
    hipFuncAttributes at;
    for (const void* k : rows) { if (hipFuncGetAttributes(&at, k) != hipSuccess) return false; if ((size_t)at.sharedSizeBytes > s.row) s.row = (size_t)at.sharedSizeBytes; }
    for (const void* k : cols) { if (hipFuncGetAttributes(&at, k) != hipSuccess) return false; if ((size_t)at.sharedSizeBytes > s.col) s.col = (size_t)at.sharedSizeBytes; }
    s.known = true;
    out = s;
    return true;
}
static const FftStaticLds* loss_fft_static_lds() {           // bnerv_loss_fwd_bwd: one launch per kernel, or the merged head / mid / coarse
    static FftStaticLds s;
    return fft_static_lds({(const void*)&fft_rows_fwd_kernel, (const void*)&fft_rows_adj_kernel, (const void*)&loss_head_kernel, (const void*)&loss_coarse_kernel},
                          {(const void*)&fft_cols_kernel, (const void*)&loss_mid_kernel}, s) ? &s : nullptr;
}
static const FftStaticLds* ssim_fft_static_lds() {           // bnerv_loss_ssim_fwd_bwd
    static FftStaticLds s;
    return fft_static_lds({(const void*)&ssim_fft_rows_fwd_kernel, (const void*)&ssim_fft_rows_adj_kernel}, {(const void*)&ssim_fft_cols_kernel}, s) ? &s : nullptr;
}

// the spectral term's launch data.  maxr: the radix limit of the caller's kernel instantiations; bc_grid_y: its column launch always has B * C as grid.y;
// sl: the static LDS of its kernels.  A frame whose lines and tables do not fit a block's LDS NEXT TO those static bytes is refused here, before any launch.
struct FftLaunch { FftArgs a; size_t lds_row, lds_col; int nrowblk; };
static int fft_launch_args(const LossCall& c, float* ws, const WsLayout& L, int maxr, size_t row_lds_limit, const FftStaticLds* sl, bool bc_grid_y, const char* who, FftLaunch& F) {
    const bnerv_loss_desc& d = c.d;
    if (sl == nullptr) return bnerv_set_error(BNERV_E_LAUNCH, "%s: the static LDS size of the FFT kernels could not be read", who);
    FftArgs& a = F.a;
    if (!make_plan(d.W, &a.prow, maxr) || !make_plan(d.H, &a.pcol, maxr))
        return bnerv_set_error(BNERV_E_ARG, "%s: FFT size %dx%d has a prime factor > %d", who, d.H, d.W, maxr);
    BNERV_REQUIRE(!bc_grid_y || c.BC <= 65535, "%s: B * C > 65535 with a spectral term", who);
    a.pred = d.pred; a.target = d.target; a.T = reinterpret_cast<float2*>(ws + L.T); a.Wh = d.W / 2 + 1; a.partial = ws + L.fft_part; a.grad = d.grad;
    a.BC = c.BC; a.H = d.H; a.W = d.W; a.gscale = d.c_fft / ((float)d.B * (float)c.nps * 2.0f); a.accumulate = 0;
    F.lds_row = (size_t)(LINES_PER_BLOCK + 1) * d.W * sizeof(float2) + (size_t)d.W * sizeof(int); F.lds_col = (size_t)(COLS_PER_BLOCK + 1) * d.H * sizeof(float2);   // + twiddle table (+ position table)
    BNERV_REQUIRE(F.lds_row + sl->row <= row_lds_limit && F.lds_col + sl->col <= FFT_LDS_PER_BLOCK,
                  "%s: frame %dx%d too large for the LDS FFT (rows %zu + %zu static bytes of %zu, columns %zu + %zu of %zu)", who, d.H, d.W,
                  F.lds_row, sl->row, row_lds_limit, F.lds_col, sl->col, FFT_LDS_PER_BLOCK);
    F.nrowblk = cdiv(c.BC * d.H, ROWS_PER_BLOCK);
    return BNERV_OK;
}
// (msval, c_ms): the MS-SSIM values and coefficient, or the single-scale path's plane values and c_ss -- the same combine
static FinalArgs final_args(const LossCall& c, float* ws, const WsLayout& L, const float* msval, float c_ms) {
    const bnerv_loss_desc& d = c.d;
    FinalArgs f{};
    f.stats_part = ws + L.stats_part; f.msval = msval; f.fft_part = d.c_fft != 0.f ? ws + L.fft_part : nullptr;
    f.loss_out = d.loss_out; f.stats_out = d.stats_out; f.B = d.B; f.C = d.C; f.n_per_sample = c.nps; f.ncolblk = L.ncolblk;
    f.c_l1 = d.c_l1; f.c_l2 = d.c_l2; f.c_ms = c_ms; f.c_fft = d.c_fft;
    return f;
}

// =====================================================================================================================
// launch paths
// =====================================================================================================================
static bool loss_fused() {                              // BNERV_LOSS_FUSED=0: the level-by-level MS-SSIM launches (A/B switch, read per call: tests compare the forms)
    return !switch_off("BNERV_LOSS_FUSED");
}
static bool even_pyramid(const WsLayout& L) {         // every pooled level has even sides: no padding anywhere, aligned 2x2 cells
    if (!loss_fused()) return false;
    for (int l = 0; l < LV - 1; ++l) if ((L.pyr.H[l] & 1) || (L.pyr.W[l] & 1)) return false;
    return true;
}
static bool adj_late() {                                // BNERV_LOSS_ADJ=late: round 4's order -- the adjoint row pass as the LAST launch, accumulating
    const char* e = switch_str("BNERV_LOSS_ADJ");       // onto the finished SSIM gradient (A/B switch, read per call; the gradient differs in the last bit:
    return e && !strcmp(e, "late");                     // fma(k, r, d) there, d + k r here)
}
static bool loss_merged() {                             // BNERV_LOSS_MERGED=0: every launch of the even-pyramid form on its own (A/B switch, read per call)
    return !switch_off("BNERV_LOSS_MERGED");
}
// the 2x2 means of an ODD pyramid, level by level (zero padding where a side is odd, count_include_pad)
static int launch_pools(hipStream_t st, const float* X, const float* Y, float* ws, const WsLayout& L) {
    const float* Xl = X; const float* Yl = Y;
    for (int l = 0; l < LV - 1; ++l) {
        const int Hl = L.pyr.H[l], Wl = L.pyr.W[l], Ho = L.pyr.H[l + 1], Wo = L.pyr.W[l + 1];
        const size_t n = (size_t)L.BC * Ho * Wo;
        int gx = (int)((n + 255) / 256); if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(avgpool2_kernel, dim3(gx, 1, 2), dim3(256), 0, st, Xl, Yl, ws + L.pyrX[l + 1], ws + L.pyrY[l + 1], L.BC, Hl, Wl, Ho, Wo, Hl % 2, Wl % 2);
        BNERV_LAUNCH_CHECK("avgpool2");
        Xl = ws + L.pyrX[l + 1]; Yl = ws + L.pyrY[l + 1];
    }
    return BNERV_OK;
}

// The pyramid, the statistics, the coefficients.  Fused: 3 launches on an even pyramid, 6 on an odd one (1080 -> 540 -> 270 -> 135 -> 68: the
// padded 2x2 means stay a launch per level) -- every level's statistics share ONE launch, the same body per tile as the level-by-level launches.
// BNERV_LOSS_FUSED=0: a statistics launch per level, 10 launches; level l's statistics read only level l's images, so the pools may all go first.
static int run_ms_forward(hipStream_t st, const float* X, const float* Y, float* ws, const WsLayout& L, float chain, bool want_g) {
    PyrArgs pa{}; SsimAllArgs sa{};
    int rc = ms_forward_args(X, Y, ws, L, want_g, pa, sa);
    if (rc) return rc;
    if (even_pyramid(L)) {
        hipLaunchKernelGGL(pyramid_kernel, dim3(cdiv(L.pyr.W[1], 16), cdiv(L.pyr.H[1], 16), 2 * L.BC), dim3(256), 0, st, pa);
        BNERV_LAUNCH_CHECK("pyramid");
    } else { rc = launch_pools(st, X, Y, ws, L); if (rc) return rc; }
    if (loss_fused()) {
        hipLaunchKernelGGL(ssim_fwd_all_kernel, dim3(sa.first[LV], L.BC), dim3(256), 0, st, sa);
        BNERV_LAUNCH_CHECK("ssim_fwd_all");
    } else {
        for (int l = 0; l < LV; ++l) {
            const dim3 grid(sa.lv[l].tiles_x, sa.lv[l].tiles_y, L.BC);
            if (l == LV - 1) hipLaunchKernelGGL(ssim_fwd_kernel<true>, grid, dim3(256), 0, st, sa.lv[l]);
            else hipLaunchKernelGGL(ssim_fwd_kernel<false>, grid, dim3(256), 0, st, sa.lv[l]);
            BNERV_LAUNCH_CHECK("ssim_fwd");
        }
    }
    hipLaunchKernelGGL(ms_coef_kernel, dim3(L.BC), dim3(320), 0, st, coef_args(ws, L, chain));
    BNERV_LAUNCH_CHECK("ms_coef");
    return BNERV_OK;
}

// acc: the level-0 launch adds to `grad` (the spectral gradient is already there) instead of writing it
static int run_ms_backward(hipStream_t st, const float* X, const float* Y, float* grad, float* ws, const WsLayout& L, float k_l1, float k_l2, int acc) {
    if (loss_fused()) {
        // 2 launches instead of 5: the coarser levels' own terms together, then level 0 with the 0.25-chain over them (odd pyramids too:
        // the chain walks the padded cells, CoarseChain::ph / pw)
        SsimAllArgs sa{};
        CoarseChain cc{};
        ms_backward_args(X, Y, grad, ws, L, k_l1, k_l2, acc, sa, cc);
        hipLaunchKernelGGL(ssim_bwd_coarse_all_kernel, dim3(sa.first[LV], L.BC), dim3(256), 0, st, sa);
        BNERV_LAUNCH_CHECK("ssim_bwd_coarse_all");
        hipLaunchKernelGGL(ssim_bwd_level0_chain_kernel, dim3(cdiv(L.pyr.W[0], STW), cdiv(L.pyr.H[0], STH), L.BC), dim3(256), 0, st, sa.lv[0], cc);
        BNERV_LAUNCH_CHECK("ssim_bwd_level0");
        return BNERV_OK;
    }
    for (int l = LV - 1; l >= 0; --l) {
        SsimArgs a = level_args(X, Y, grad, ws, L, l);
        if (l < LV - 1) { a.dcoarse = ws + L.dXl[l + 1]; a.Hc = L.pyr.H[l + 1]; a.Wc = L.pyr.W[l + 1]; a.ph = a.H % 2; a.pw = a.W % 2; }
        if (l == 0) { a.k_l1 = k_l1; a.k_l2 = k_l2; a.acc = acc; }
        const dim3 grid(cdiv(a.W, STW), cdiv(a.H, STH), L.BC);
        if (l == 0) hipLaunchKernelGGL((ssim_bwd_from_g_kernel<true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ssim_bwd_from_g_kernel<false>), grid, dim3(256), 0, st, a);
        BNERV_LAUNCH_CHECK("ssim_bwd");
    }
    return BNERV_OK;
}

static int launch_stats(hipStream_t st, const float* p, const float* t, float* part, int B, int n_per_sample) {
    hipLaunchKernelGGL(diff_stats_kernel, dim3(NSB, B), dim3(256), 0, st, p, t, part, n_per_sample);
    BNERV_LAUNCH_CHECK("diff_stats");
    return BNERV_OK;
}

}  // namespace

extern "C" size_t bnerv_loss_ws_bytes(int B, int C, int H, int W, int use_ms, int use_fft) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return make_layout(B, C, H, W, use_ms ? LV : 0, use_fft != 0).total * sizeof(float);
}

// (A second stream for the spectral branch was measured and dropped: forked with an event pair the loss section of the trace shrinks
// from 207 to 194 us, but the column FFT doubles next to the SSIM maps, the fork / join edges idle the chip for 6 + 10 us and a
// two-branch graph replays slower than a linear one: C1 1.789 ms forked against 1.759 ms.  Independent launches are merged as block
// ranges of one grid instead -- loss_head / loss_mid / loss_tail above.)
extern "C" int bnerv_loss_fwd_bwd(void* stream, const bnerv_loss_desc* dp) {
    LossCall c;
    if (const int rc_d = open_loss_call(dp, "loss", c)) return rc_d;
    const bnerv_loss_desc& d = c.d;
    const bool use_ms = d.c_ms != 0.f, use_fft = d.c_fft != 0.f;
    const WsLayout L = make_layout(d.B, d.C, d.H, d.W, use_ms ? LV : 0, use_fft);
    if (d.ws_bytes < L.total * sizeof(float)) return bnerv_set_error(BNERV_E_WS, "loss: workspace %zu < %zu", d.ws_bytes, L.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(d.ws);
    const int BC = c.BC;
    if (use_ms && (d.H <= 160 || d.W <= 160)) return bnerv_set_error(BNERV_E_ARG, "loss: MS-SSIM needs min(H,W) > 160 (got %dx%d)", d.H, d.W);
    FftLaunch F{};
    if (use_fft) {
        if (const int rc_f = fft_launch_args(c, ws, L, BNERV_FFT_MAX_RADIX, FFT_LDS_PER_BLOCK, loss_fft_static_lds(), false, "loss", F)) return rc_f;
        F.a.accumulate = 1;
    }
    const FinalArgs f = final_args(c, ws, L, use_ms ? ws + L.msval : nullptr, d.c_ms);
    const float chain = -d.c_ms / (float)BC;

    const bool late = adj_late();
    if (use_ms && use_fft && d.grad && loss_fused() && loss_merged()) {
        // 5 launches on an even pyramid (9 on an odd one, whose four pooled levels are a launch each): head (row FFTs | pyramid | L1 / L2 sums),
        // SSIM statistics, mid (column FFTs | coefficients), coarse (adjoint row FFTs -> the spectral gradient | coarse SSIM gradients),
        // tail (level-0 gradient, added to the spectral one | loss_final).  BNERV_LOSS_ADJ=late: the adjoint rows as a sixth launch behind the tail.
        const bool even = even_pyramid(L);
        LossHeadArgs ha{}; LossMidArgs ma{}; LossTailArgs ta{};
        SsimAllArgs sf{};
        int rc = ms_forward_args(d.pred, d.target, ws, L, true, ha.p, sf);
        if (rc) return rc;
        ha.f = F.a; ha.pred = d.pred; ha.target = d.target; ha.stats_part = ws + L.stats_part; ha.nps = c.nps;
        ha.n_fft = F.nrowblk; ha.pyr_gx = cdiv(L.pyr.W[1], 16); ha.pyr_gy = cdiv(L.pyr.H[1], 16); ha.n_pyr = even ? ha.pyr_gx * ha.pyr_gy * 2 * BC : 0;
        if (const int rc_lds = dyn_lds<&loss_head_kernel>(F.lds_row, "loss_head")) return rc_lds;
        hipLaunchKernelGGL(loss_head_kernel, dim3(ha.n_fft + ha.n_pyr + NSB * d.B), dim3(256), F.lds_row, st, ha);
        BNERV_LAUNCH_CHECK("loss_head");
        if (!even) { rc = launch_pools(st, d.pred, d.target, ws, L); if (rc) return rc; }
        hipLaunchKernelGGL(ssim_fwd_all_kernel, dim3(sf.first[LV], BC), dim3(256), 0, st, sf);
        BNERV_LAUNCH_CHECK("ssim_fwd_all");
        ma.f = F.a; ma.c = coef_args(ws, L, chain); ma.ncolblk = L.ncolblk; ma.n_cols = L.ncolblk * BC;
        if (const int rc_lds = dyn_lds<&loss_mid_kernel>(F.lds_col, "loss_mid")) return rc_lds;
        hipLaunchKernelGGL(loss_mid_kernel, dim3(ma.n_cols + BC), dim3(256), F.lds_col, st, ma);
        BNERV_LAUNCH_CHECK("loss_mid");
        SsimAllArgs sb{};
        ms_backward_args(d.pred, d.target, d.grad, ws, L, c.k_l1, c.k_l2, late ? 0 : 1, sb, ta.cc);
        if (late) {
            hipLaunchKernelGGL(ssim_bwd_coarse_all_kernel, dim3(sb.first[LV], BC), dim3(256), 0, st, sb);
            BNERV_LAUNCH_CHECK("ssim_bwd_coarse_all");
        } else {
            LossCoarseArgs ca{};
            ca.f = F.a; ca.f.accumulate = 0; ca.s = sb; ca.n_adj = F.nrowblk; ca.gx = sb.first[LV]; ca.BC = BC;
            const size_t lds_c = F.lds_row > SSIM_BWD_LDS * sizeof(float) ? F.lds_row : SSIM_BWD_LDS * sizeof(float);
            if (const int rc_lds = dyn_lds<&loss_coarse_kernel>(lds_c, "loss_coarse")) return rc_lds;
            hipLaunchKernelGGL(loss_coarse_kernel, dim3(ca.n_adj + ca.gx * BC), dim3(256), lds_c, st, ca);
            BNERV_LAUNCH_CHECK("loss_coarse");
        }
        ta.s = sb.lv[0]; ta.fin = f; ta.gx = cdiv(L.pyr.W[0], STW); ta.gy = cdiv(L.pyr.H[0], STH); ta.BC = BC; ta.n0 = ta.gx * ta.gy * BC;
        hipLaunchKernelGGL(loss_tail_kernel, dim3(ta.n0 + 1), dim3(256), 0, st, ta);
        BNERV_LAUNCH_CHECK("loss_tail");
        if (late) {
            if (const int rc_lds = dyn_lds<&fft_rows_adj_kernel>(F.lds_row, "fft_rows_adj")) return rc_lds;
            hipLaunchKernelGGL(fft_rows_adj_kernel, dim3(F.nrowblk), dim3(256), F.lds_row, st, F.a);
            BNERV_LAUNCH_CHECK("fft_rows_adj");
        }
        return BNERV_OK;
    }

    // one launch per kernel.  With both an MS-SSIM and a spectral term the spectral gradient is written FIRST and the level-0 SSIM launch adds
    // to it -- the arithmetic of the merged form above, so the two forms agree bit for bit (BNERV_LOSS_ADJ=late: the other order, in both forms)
    const bool fft_first = use_ms && use_fft && d.grad && !late;
    int rc = launch_stats(st, d.pred, d.target, ws + L.stats_part, d.B, c.nps);
    if (rc) return rc;
    auto run_fft = [&](int accumulate) -> int {
        FftArgs fa = F.a; fa.accumulate = accumulate;
        if (const int rc_lds = dyn_lds<&fft_rows_fwd_kernel>(F.lds_row, "fft_rows_fwd")) return rc_lds;
        if (const int rc_lds = dyn_lds<&fft_rows_adj_kernel>(F.lds_row, "fft_rows_adj")) return rc_lds;
        if (const int rc_lds = dyn_lds<&fft_cols_kernel>(F.lds_col, "fft_cols")) return rc_lds;
        hipLaunchKernelGGL(fft_rows_fwd_kernel, dim3(F.nrowblk), dim3(256), F.lds_row, st, fa);
        BNERV_LAUNCH_CHECK("fft_rows_fwd");
        hipLaunchKernelGGL(fft_cols_kernel, dim3(L.ncolblk, BC), dim3(256), F.lds_col, st, fa);
        BNERV_LAUNCH_CHECK("fft_cols");
        if (d.grad) {
            hipLaunchKernelGGL(fft_rows_adj_kernel, dim3(F.nrowblk), dim3(256), F.lds_row, st, fa);
            BNERV_LAUNCH_CHECK("fft_rows_adj");
        }
        return BNERV_OK;
    };
    if (use_ms) {
        rc = run_ms_forward(st, d.pred, d.target, ws, L, chain, d.grad != nullptr);
        if (rc) return rc;
        if (fft_first) { rc = run_fft(0); if (rc) return rc; }
        if (d.grad) { rc = run_ms_backward(st, d.pred, d.target, d.grad, ws, L, c.k_l1, c.k_l2, fft_first ? 1 : 0); if (rc) return rc; }
    } else if (d.grad) {
        const size_t n = (size_t)d.B * c.nps;
        int gx = (int)((n + 1023) / 1024); if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(grad_l1l2_kernel, dim3(gx), dim3(256), 0, st, d.pred, d.target, d.grad, n, c.k_l1, c.k_l2);
        BNERV_LAUNCH_CHECK("grad_l1l2");
    }
    if (use_fft && !fft_first) { rc = run_fft(1); if (rc) return rc; }
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, st, f);
    BNERV_LAUNCH_CHECK("loss_final");
    return BNERV_OK;
}

extern "C" int bnerv_msssim(void* stream, const float* x, const float* y, float* out, void* wsv, size_t ws_bytes, int B, int C, int H, int W) {
    BNERV_REQUIRE(x && y && out && wsv && B > 0 && C > 0, "msssim: bad args");
    if (H <= 160 || W <= 160) return bnerv_set_error(BNERV_E_ARG, "msssim: needs min(H,W) > 160 (got %dx%d)", H, W);
    const WsLayout L = make_layout(B, C, H, W, LV, false);
    if (ws_bytes < L.total * sizeof(float)) return bnerv_set_error(BNERV_E_WS, "msssim: workspace %zu < %zu", ws_bytes, L.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(wsv);
    int rc = run_ms_forward(st, x, y, ws, L, 0.f, false);
    if (rc) return rc;
    hipLaunchKernelGGL(msssim_final_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, ws + L.msval, out, B, C);
    BNERV_LAUNCH_CHECK("msssim_final");
    return BNERV_OK;
}

extern "C" size_t bnerv_loss_ssim_ws_bytes(int B, int C, int H, int W, int use_fft) {
    if (B <= 0 || C <= 0 || H <= HW_ || W <= HW_) return 0;
    return make_layout(B, C, H, W, 1, use_fft != 0).total * sizeof(float);
}

// The single-scale SSIM losses: the descriptor of bnerv_loss_fwd_bwd plus c_ssim (c_ms must be 0).  2 launches (5 with a spectral term).
extern "C" int bnerv_loss_ssim_fwd_bwd(void* stream, const bnerv_loss_desc* dp, float c_ssim) {
    LossCall c;
    if (const int rc_d = open_loss_call(dp, "loss_ssim", c)) return rc_d;
    const bnerv_loss_desc& d = c.d;
    BNERV_REQUIRE(d.c_ms == 0.f, "loss_ssim: c_ms must be 0 (the MS-SSIM losses go through bnerv_loss_fwd_bwd)");
    BNERV_REQUIRE(c_ssim != 0.f, "loss_ssim: c_ssim is 0 (losses without an SSIM term go through bnerv_loss_fwd_bwd)");
    if (d.H <= HW_ || d.W <= HW_) return bnerv_set_error(BNERV_E_ARG, "loss_ssim: SSIM needs min(H,W) >= %d (got %dx%d)", WS_, d.H, d.W);
    const bool use_fft = d.c_fft != 0.f;
    const WsLayout L = make_layout(d.B, d.C, d.H, d.W, 1, use_fft);
    if (d.ws_bytes < L.total * sizeof(float)) return bnerv_set_error(BNERV_E_WS, "loss_ssim: workspace %zu < %zu", d.ws_bytes, L.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(d.ws);
    const int BC = c.BC;
    BNERV_REQUIRE((size_t)L.tiles[0] * BC + (size_t)BC * d.H + (size_t)NSB * d.B < (size_t)1 << 30, "loss_ssim: batch too large for one grid");
    FftLaunch F{};
    if (use_fft) {
        if (const int rc_f = fft_launch_args(c, ws, L, SSIM_FFT_MAX_RADIX, 128 * 1024, ssim_fft_static_lds(), true, "loss_ssim", F)) return rc_f;
        if (const int rc_lds = dyn_lds<&ssim_fft_rows_fwd_kernel>(F.lds_row, "ssim_fft_rows_fwd")) return rc_lds;
        hipLaunchKernelGGL(ssim_fft_rows_fwd_kernel, dim3(F.nrowblk), dim3(256), F.lds_row, st, F.a);
        BNERV_LAUNCH_CHECK("ssim_fft_rows_fwd");
    }
    SsimHeadArgs ha{};
    ha.s = level_args(d.pred, d.target, d.grad, ws, L, 0);
    if (!d.grad) ha.s.G = nullptr;
    ha.s.coef = nullptr; ha.s.coef_k = (-c_ssim / (float)BC) * inv_nvalid(L, 0); ha.s.k_l1 = c.k_l1; ha.s.k_l2 = c.k_l2; ha.s.acc = use_fft ? 1 : 0;
    ha.pred = d.pred; ha.target = d.target; ha.stats_part = ws + L.stats_part; ha.nps = c.nps; ha.n_sums = NSB * d.B; ha.BC = BC;
    hipLaunchKernelGGL(ssim_head_kernel, dim3(ha.n_sums + L.tiles[0] * BC), dim3(256), 0, st, ha);
    BNERV_LAUNCH_CHECK("ssim_head");
    if (use_fft) {
        if (const int rc_lds = dyn_lds<&ssim_fft_cols_kernel>(F.lds_col, "ssim_fft_cols")) return rc_lds;
        hipLaunchKernelGGL(ssim_fft_cols_kernel, dim3(L.ncolblk, BC), dim3(256), F.lds_col, st, F.a);
        BNERV_LAUNCH_CHECK("ssim_fft_cols");
        if (d.grad) {                                                      // the spectral gradient, WRITTEN: the tail adds to it
            if (const int rc_lds = dyn_lds<&ssim_fft_rows_adj_kernel>(F.lds_row, "ssim_fft_rows_adj")) return rc_lds;
            hipLaunchKernelGGL(ssim_fft_rows_adj_kernel, dim3(F.nrowblk), dim3(256), F.lds_row, st, F.a);
            BNERV_LAUNCH_CHECK("ssim_fft_rows_adj");
        }
    }
    SsimTailArgs ta{};
    ta.s = ha.s;
    ta.fin = SsimFinalArgs{ws + L.ssim_part[0], ws + L.msval, inv_nvalid(L, 0), L.tiles[0], BC, final_args(c, ws, L, ws + L.msval, c_ssim)};
    if (d.grad) {
        ta.gx = cdiv(d.W, STW); ta.gy = cdiv(d.H, STH); ta.BC = BC; ta.n0 = ta.gx * ta.gy * BC;
        hipLaunchKernelGGL(ssim_tail_kernel, dim3(ta.n0 + 1), dim3(256), 0, st, ta);
        BNERV_LAUNCH_CHECK("ssim_tail");
    } else {
        hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, st, ta.fin);
        BNERV_LAUNCH_CHECK("ssim_final");
    }
    return BNERV_OK;
}

// per-sample SSIM only: out [B]; ws: bnerv_loss_ssim_ws_bytes(B, C, H, W, 0)
extern "C" int bnerv_ssim(void* stream, const float* x, const float* y, float* out, void* wsv, size_t ws_bytes, int B, int C, int H, int W) {
    BNERV_REQUIRE(x && y && out && wsv && B > 0 && C > 0, "ssim: bad args");
    if (H <= HW_ || W <= HW_) return bnerv_set_error(BNERV_E_ARG, "ssim: needs min(H,W) >= %d (got %dx%d)", WS_, H, W);
    const WsLayout L = make_layout(B, C, H, W, 1, false);
    if (ws_bytes < L.total * sizeof(float)) return bnerv_set_error(BNERV_E_WS, "ssim: workspace %zu < %zu", ws_bytes, L.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(wsv);
    const int BC = B * C;
    BNERV_REQUIRE(BC <= 65535, "ssim: batch too large");
    SsimArgs a = level_args(x, y, nullptr, ws, L, 0);
    a.G = nullptr; a.coef = nullptr;
    hipLaunchKernelGGL(ssim_fwd_kernel<true>, dim3(a.tiles_x, a.tiles_y, BC), dim3(256), 0, st, a);
    BNERV_LAUNCH_CHECK("ssim_fwd");
    const SsimFinalArgs sf{ws + L.ssim_part[0], ws + L.msval, inv_nvalid(L, 0), L.tiles[0], BC};
    hipLaunchKernelGGL(ssim_metric_kernel, dim3(1), dim3(256), 0, st, sf, out, B, C);
    BNERV_LAUNCH_CHECK("ssim_metric");
    return BNERV_OK;
}

extern "C" size_t bnerv_psnr_ws_bytes(int B, int C, int H, int W) { return B > 0 ? make_layout(B, C, H, W, 0, false).total * sizeof(float) : 0; }

extern "C" int bnerv_psnr(void* stream, const float* o, const float* gt, float* psnr, void* ws, size_t ws_bytes, int B, int C, int H, int W) {
    BNERV_REQUIRE(o && gt && psnr && ws && B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "psnr: bad args");
    BNERV_REQUIRE((size_t)C * H * W < (size_t)1 << 31, "psnr: sample too large");
    if (ws_bytes < bnerv_psnr_ws_bytes(B, C, H, W)) return bnerv_set_error(BNERV_E_WS, "psnr: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_stats(st, o, gt, (float*)ws, B, C * H * W);
    if (rc) return rc;
    hipLaunchKernelGGL(psnr_final_kernel, dim3(B), dim3(64), 0, st, (const float*)ws, psnr, B, C * H * W);
    BNERV_LAUNCH_CHECK("psnr_final");
    return BNERV_OK;
}

// Create the FFT twiddle tables for an H x W frame ahead of time (they are otherwise created on first use; creation
// allocates and copies synchronously, which is illegal inside a stream capture).
extern "C" int bnerv_fft_prepare(int H, int W) {
    FftPlan p;
    if (!make_plan(H, &p) || !make_plan(W, &p)) return bnerv_set_error(BNERV_E_ARG, "fft_prepare: %dx%d has a prime factor > %d", H, W, BNERV_FFT_MAX_RADIX);
    (void)loss_fft_static_lds();                          // (read here so that a captured call finds it cached; a failure is reported by that call)
    return BNERV_OK;
}

// The same for bnerv_loss_ssim_fwd_bwd with a spectral term, whose instantiations take prime factors up to SSIM_FFT_MAX_RADIX.
extern "C" int bnerv_loss_ssim_prepare(int H, int W) {
    FftPlan p;
    if (!make_plan(H, &p, SSIM_FFT_MAX_RADIX) || !make_plan(W, &p, SSIM_FFT_MAX_RADIX))
        return bnerv_set_error(BNERV_E_ARG, "loss_ssim_prepare: %dx%d has a prime factor > %d", H, W, SSIM_FFT_MAX_RADIX);
    (void)ssim_fft_static_lds();
    return BNERV_OK;
}
