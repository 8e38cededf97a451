// conv5.hip -- the 5x5 'same' convolution family of the HNeRV baseline decoder (gfx950): forward, data gradient, weight + bias gradient.
//
// Reference call sites: UpConv 'pshuffel' with ks = 5 (model_blocks.py:196-220: CustomConv2d 5x5 + PixelShuffle) followed by GELU inside
// NeRVBlock (model_blocks.py:34-46), as built by HNeRV.__init__ (model_hnerv.py:49-56) for `--conv_type convnext pshuffel --ks 0_1_5`,
// and autograd's backward of the same.  f32 contract on the 16-bit matrix pipe: every f32 operand is split into bf16 pieces
// (split16.h; convbf.hip explains the scheme) and v_mfma_f32_16x16x32_bf16 accumulates the six piece products in f32.
//
// Forward / data gradient (conv5_kernel).  GEMM view: M = 16 couts, N = 16 pixels of one image row, K = (tap, channel) in steps of 32 =
// two taps x 16 channels; lane (i = l & 15, kq = l >> 4) holds tap 2 s + (kq >> 1), channels 8 (kq & 1) .. + 7.  25 taps = 13 steps, the
// 26th tap carries zero weights.
//   * block = 8 x 32 pixels x 64 couts x all Cin (16-channel chunks); 4 waves = 2 (row halves) x 2 (cout tile pairs); a wave keeps
//     8 pixel tiles x 2 cout tiles = 64 accumulator registers;
//   * pixel operand: the 12 x 36 halo tile of a chunk, transformed (pixel-unshuffle gather, optional product with a saved GELU'), split,
//     and stored PIXEL-MAJOR in LDS -- s_a[piece][row][pixel][half], 16-byte slots of 8 channels -- 3 x 13.5 KiB = 40.5 KiB;
//   * weight operand: fragments in lane order in GLOBAL memory (caller's workspace), written by conv5_wprep_kernel before the main
//     launch; a wave reads its two cout tiles' fragments with one 16-byte load per (step, piece) -- they stay in L2 (1.2 MB for the
//     largest H1 layer).  LDS holds no weights: 39 KiB per cout tile and chunk would not fit beside the image;
//   * accumulators: mfma(weights, pixels) -> lane holds pixel l & 15 and the 4 consecutive couts 4 (l >> 4) .. + 3: with PixelShuffle(2)
//     these are the 2 x 2 output block of ONE output channel (two 8-byte stores, lanes consecutive in x).
//
// Weight gradient (wgrad5_kernel).  K = pixels (32 = one tile row per MFMA), M = 16 couts, N = 16 cins, one accumulator per tap:
//   * block = 128 couts x 16 cins x a strided share of the 8 x 32 tiles; wave w owns cout tiles 2 w, 2 w + 1 -> 2 x 25 accumulators;
//   * the gradient operand goes global -> registers (unshuffle gather, optional GELU' product, split there), no redundancy across waves;
//   * the input operand is the split halo tile CHANNEL-MAJOR in LDS, s_x[piece][channel][row][pixel] bf16; a tap's fragment is 8
//     consecutive pixels at a 2-byte-aligned address (gfx950 LDS serves unaligned 16-byte reads);
//   * bias gradient: one more accumulator against a fragment of ones (ci chunk 0 only);
//   * every block writes its share as a slab [tap][cout][cin]; wgrad5_reduce_kernel sums the slabs in a fixed order and transposes to OIHW.
#include "common.h"
#include "split16.h"
#include "launch.h"

namespace {

constexpr int C5_K = 5, C5_T = 25, C5_PAD = 2, C5_STEPS = 13;
constexpr int C5_TH = 8, C5_TW = 32, C5_ROWS = C5_TH + 2 * C5_PAD, C5_NP = C5_TW + 2 * C5_PAD;      // 12 halo rows x 36 pixels
constexpr int C5_PIECE = C5_ROWS * C5_NP * 2 * 16;                                                  // bytes of one piece: 13824
constexpr int C5_NTB = 4;                                                                           // cout tiles per block

// BNERV_SPLIT_WIDE picks the arithmetic as for the wide 3x3 kernels (split_wide_mode(), launch.h); there is no f32 5x5 kernel, so "off" runs bf16x6
static bool c5_x3() { return split_wide_mode() == SP_BF16X3; }

struct C5Args {
    bnerv_conv_desc d;
    const u32x4* wfrag;
    int tiles_x, tiles_y, nchunk, ntile, ngroup;
};

// weight fragments: frag[((chunk * ntile + ct) * 13 + step) * NS + piece][lane]
template <int SP>
__global__ __launch_bounds__(256) void conv5_wprep_kernel(const float* __restrict__ w, u32x4* __restrict__ frag, const int Cin, const int Cout,
                                                          const int wCi, const int transposed, const int nchunk, const int ntile) {
    constexpr int NS = Split<SP>::NS;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = nchunk * ntile * C5_STEPS * 64;
    if (idx >= total) return;
    const int lane = idx & 63, r = idx >> 6;
    const int s = r % C5_STEPS, q = r / C5_STEPS;
    const int ct = q % ntile, chunk = q / ntile;
    const int co = ct * 16 + (lane & 15), kq = lane >> 4;
    const int t = 2 * s + (kq >> 1);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ci = chunk * 16 + 8 * (kq & 1) + e;
        float x = 0.f;
        if (co < Cout && ci < Cin && t < C5_T)
            x = transposed ? w[((size_t)ci * wCi + co) * C5_T + (C5_T - 1 - t)] : w[((size_t)co * wCi + ci) * C5_T + t];
        v[e] = x;
    }
    u32x4 pc[NS];
    split8<SP, 8>(v, pc);
#pragma unroll
    for (int p = 0; p < NS; ++p) frag[((size_t)r * NS + p) * 64 + lane] = pc[p];
}

template <int SP>
__global__ __launch_bounds__(256, 2) void conv5_kernel(const C5Args ka) {
    constexpr int NS = Split<SP>::NS;
    const bnerv_conv_desc& d = ka.d;
    extern __shared__ __attribute__((aligned(16))) char s_a[];                // [NS][C5_PIECE]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 15, kq = lane >> 4;
    const int Cin = d.Cin, Cout = d.Cout, H = d.H, W = d.W;

    int bid = blockIdx.x;
    const int grp = bid % ka.ngroup; bid /= ka.ngroup;
    const int tx = bid % ka.tiles_x; bid /= ka.tiles_x;
    const int ty = bid % ka.tiles_y;
    const int b = bid / ka.tiles_y;
    const int y0 = ty * C5_TH, x0 = tx * C5_TW;
    const int ct0 = grp * C5_NTB + 2 * wn;                                    // this wave's cout tiles ct0, ct0 + 1
    const bool has0 = ct0 < ka.ntile, has1 = ct0 + 1 < ka.ntile;              // (wave-uniform)

    f32x4 acc[8][2];
#pragma unroll
    for (int m = 0; m < 8; ++m) { acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[m][1] = acc[m][0]; }

    const int in_s = d.in_mode == BNERV_IN_UNSHUFFLE ? d.in_s : 1;
    const int ss = in_s * in_s, Cs = Cin / ss, Hs = H * in_s, Ws = W * in_s;  // stored shape [B, Cs, Hs, Ws]
    const float* __restrict__ xb = d.x + (size_t)b * Cin * H * W;
    const float* __restrict__ ab = d.aux0 ? d.aux0 + (size_t)b * Cin * H * W : nullptr;

    for (int chunk = 0; chunk < ka.nchunk; ++chunk) {
        if (chunk) __syncthreads();                                          // every wave is done reading the previous chunk
        // ---- staging: slot = (half, row, pixel): 8 channels of one pixel -> NS 16-byte pieces
        for (int slot = tid; slot < 2 * C5_ROWS * C5_NP; slot += 256) {
            const int p = slot % C5_NP, rh = slot / C5_NP;
            const int r = rh % C5_ROWS, h = rh / C5_ROWS;
            const int gy = y0 + r - C5_PAD, gx = x0 + p - C5_PAD;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = chunk * 16 + 8 * h + e;
                float x = 0.f;
                if (inside && c < Cin) {
                    size_t off;
                    if (in_s == 1) {
                        off = ((size_t)c * H + gy) * W + gx;
                    } else {
                        const int cc = c / ss, ij = c - cc * ss, i = ij / in_s, j = ij - i * in_s;
                        off = ((size_t)cc * Hs + (gy * in_s + i)) * Ws + (gx * in_s + j);
                    }
                    x = xb[off];
                    if (ab) x *= ab[off];
                }
                v[e] = x;
            }
            u32x4 pc[NS];
            split8<SP, 8>(v, pc);
#pragma unroll
            for (int q = 0; q < NS; ++q) *reinterpret_cast<u32x4*>(s_a + q * C5_PIECE + ((r * C5_NP + p) * 2 + h) * 16) = pc[q];
        }
        __syncthreads();
        // ---- contraction
        const u32x4* __restrict__ wf0 = ka.wfrag + ((size_t)(chunk * ka.ntile + ct0) * C5_STEPS) * NS * 64 + lane;
#pragma unroll 1
        for (int s = 0; s < C5_STEPS; ++s) {
            u32x4 bfr[2][NS];
#pragma unroll
            for (int p = 0; p < NS; ++p) {
                bfr[0][p] = has0 ? wf0[((size_t)s * NS + p) * 64] : u32x4{0u, 0u, 0u, 0u};
                bfr[1][p] = has1 ? wf0[((size_t)(C5_STEPS + s) * NS + p) * 64] : u32x4{0u, 0u, 0u, 0u};
            }
            int t = 2 * s + (kq >> 1);
            t = t > C5_T - 1 ? C5_T - 1 : t;                                 // tap 25: zero weights, any finite in-tile pixel
            const int ky = t / C5_K, kx = t - ky * C5_K;
            const int abase = (((4 * wm + ky) * C5_NP + kx + li) * 2 + (kq & 1)) * 16;
            if (has0) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    u32x4 afr[NS];
#pragma unroll
                    for (int p = 0; p < NS; ++p)
                        afr[p] = *reinterpret_cast<const u32x4*>(s_a + p * C5_PIECE + abase + (((m >> 1) * C5_NP + 16 * (m & 1)) * 2) * 16);
#define BNERV_C5_PROD(pa, pb) acc[m][0] = mfma16<SP>(bfr[0][pb], afr[pa], acc[m][0]); if (has1) acc[m][1] = mfma16<SP>(bfr[1][pb], afr[pa], acc[m][1]);
                    if constexpr (NS == 3) {
                        BNERV_C5_PROD(2, 0)
                        BNERV_C5_PROD(0, 2)
                        BNERV_C5_PROD(1, 1)
                    }
                    BNERV_C5_PROD(1, 0)
                    BNERV_C5_PROD(0, 1)
                    BNERV_C5_PROD(0, 0)
#undef BNERV_C5_PROD
                }
            }
        }
    }

    // ---- epilogue: lane = pixel (row 4 wm + (m >> 1), x = 16 (m & 1) + li), couts ct * 16 + 4 kq + i
    const int ep = d.ep_mode, os = d.out_s;
    float* __restrict__ ob = d.out + (size_t)b * Cout * H * W;
    float* __restrict__ o2b = d.out2 ? d.out2 + (size_t)b * Cout * H * W : nullptr;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        if (!(n ? has1 : has0)) continue;
        const int co = (ct0 + n) * 16 + 4 * kq;
        if (co >= Cout) continue;
        float bias[4] = {0.f, 0.f, 0.f, 0.f};
        if (ep != BNERV_EP_PLAIN && d.bias) {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (co + i < Cout) bias[i] = d.bias[co + i];
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int y = y0 + 4 * wm + (m >> 1), x = x0 + 16 * (m & 1) + li;
            if (y >= H || x >= W) continue;
            float u[4], g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u[i] = acc[m][n][i] + bias[i];
                g[i] = 0.f;
                if (ep == BNERV_EP_BIAS_GELU) { float hh, gg; gelu_pair_f(u[i], &hh, &gg); u[i] = hh; g[i] = gg; }
            }
            if (os == 2) {                                                   // co = 4 cc + 2 i + j -> out[cc][2 y + i][2 x + j]  (Cout % 4 == 0)
                const size_t o = ((size_t)(co >> 2) * (2 * H) + 2 * y) * (2 * W) + 2 * x;
                *reinterpret_cast<f32x2*>(ob + o) = f32x2{u[0], u[1]};
                *reinterpret_cast<f32x2*>(ob + o + 2 * W) = f32x2{u[2], u[3]};
                if (o2b) {
                    *reinterpret_cast<f32x2*>(o2b + o) = f32x2{g[0], g[1]};
                    *reinterpret_cast<f32x2*>(o2b + o + 2 * W) = f32x2{g[2], g[3]};
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (co + i < Cout) {
                        const size_t o = ((size_t)(co + i) * H + y) * W + x;
                        ob[o] = u[i];
                        if (o2b) o2b[o] = g[i];
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
constexpr int W5_ROWB = 80;                                  // bytes per LDS row: 36 px x 2 B, padded to a multiple of 16
constexpr int W5_PLANE = C5_ROWS * W5_ROWB;                  // 960
constexpr int W5_PIECE = 16 * W5_PLANE + 16;                 // + 16: the last fragment of the last plane may read up to 14 bytes past its row
constexpr int W5_CG = 128;                                   // couts per block (2 tiles per wave)

struct W5Args {
    bnerv_wgrad_desc d;
    float* slab;                                             // [nslab][25][Cout][Cin] then [nslab][Cout]
    int tiles_x, tiles_y, ncic, ncog, nslab;
};

template <int SP>
__global__ __launch_bounds__(256) void wgrad5_kernel(const W5Args wa) {
    constexpr int NS = Split<SP>::NS;
    const bnerv_wgrad_desc& d = wa.d;
    extern __shared__ __attribute__((aligned(16))) char s_x[];               // [NS][W5_PIECE]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int Cin = d.Cin, Cout = d.Cout, H = d.H, W = d.W;

    int bid = blockIdx.x;
    const int cic = bid % wa.ncic; bid /= wa.ncic;
    const int cog = bid % wa.ncog;
    const int sl = bid / wa.ncog;
    const int co_t0 = cog * W5_CG + wave * 32;                                // first cout of this wave's two tiles
    const bool has0 = co_t0 < Cout, has1 = co_t0 + 16 < Cout;                 // (wave-uniform)
    const bool want_b = cic == 0 && d.db != nullptr;

    f32x4 acc[2][C5_T];
    f32x4 accb[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        accb[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < C5_T; ++t) acc[n][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};   // bf16 1.0 x 8

    const int g_s = d.g_mode == BNERV_IN_UNSHUFFLE ? d.g_s : 1;
    const int gss = g_s * g_s, Hs = H * g_s, Ws = W * g_s;
    const int total = d.B * wa.tiles_y * wa.tiles_x;
    // the padding bytes of the image (row tails, piece tail) are never read by a fragment; cleared once all the same so that no garbage sits in the image
    for (int i = tid; i < NS * W5_PIECE / 4; i += 256) reinterpret_cast<unsigned*>(s_x)[i] = 0u;

    for (int tile = sl; tile < total; tile += wa.nslab) {
        const int tx = tile % wa.tiles_x, r1 = tile / wa.tiles_x;
        const int ty = r1 % wa.tiles_y, b = r1 / wa.tiles_y;
        const int y0 = ty * C5_TH, x0 = tx * C5_TW;
        const float* __restrict__ xb = d.x + (size_t)b * Cin * H * W;
        const float* __restrict__ gb = d.g + (size_t)b * Cout * H * W;
        const float* __restrict__ ab = d.gaux ? d.gaux + (size_t)b * Cout * H * W : nullptr;
        __syncthreads();                                                     // previous tile's reads (and the clear) are done
        // ---- stage the input halo tile: slot = (channel, row, pixel pair) -> NS packed bf16 pairs
        for (int slot = tid; slot < 16 * C5_ROWS * (C5_NP / 2); slot += 256) {
            const int pp = slot % (C5_NP / 2), cr = slot / (C5_NP / 2);
            const int r = cr % C5_ROWS, c = cr / C5_ROWS;
            const int ci = cic * 16 + c;
            const int gy = y0 + r - C5_PAD, gx = x0 + 2 * pp - C5_PAD;
            f32x2 v = {0.f, 0.f};
            if (ci < Cin && gy >= 0 && gy < H) {
                const float* row = xb + ((size_t)ci * H + gy) * W;
                if (gx >= 0 && gx < W) v[0] = row[gx];
                if (gx + 1 >= 0 && gx + 1 < W) v[1] = row[gx + 1];
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const unsigned pk = pk16<SP>(v[0], v[1]);
                *reinterpret_cast<unsigned*>(s_x + q * W5_PIECE + c * W5_PLANE + r * W5_ROWB + pp * 4) = pk;
                if (q + 1 < NS) v -= unpk16<SP>(pk);
            }
        }
        __syncthreads();
        if (!has0) continue;                                                 // (uniform per wave; the barriers above are reached by all)
        // gradient values of one tile row: lane (co, kq) holds pixels x0 + 8 kq .. + 7.  Row r + 1 is loaded while row r's products run
        // (one wave per SIMD: nothing else would cover the latency).
        auto load_g = [&](const int gy, float (&v)[2][8]) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int co = co_t0 + 16 * n + li;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int gx = x0 + 8 * kq + e;
                    float x = 0.f;
                    if (co < Cout && gx < W && gy < H) {
                        size_t off;
                        if (g_s == 1) {
                            off = ((size_t)co * H + gy) * W + gx;
                        } else {
                            const int cc = co / gss, ij = co - cc * gss, i = ij / g_s, j = ij - i * g_s;
                            off = ((size_t)cc * Hs + (gy * g_s + i)) * Ws + (gx * g_s + j);
                        }
                        x = gb[off];
                        if (ab) x *= ab[off];
                    }
                    v[n][e] = x;
                }
            }
        };
        float gv[2][8];
        load_g(y0, gv);
#pragma unroll 1
        for (int r = 0; r < C5_TH; ++r) {
            const int gy = y0 + r;
            if (gy >= H) break;
            u32x4 gfr[2][NS];
            split8<SP, 8>(gv[0], gfr[0]);
            split8<SP, 8>(gv[1], gfr[1]);
            if (r + 1 < C5_TH) load_g(gy + 1, gv);                            // (rows >= H load nothing and give zeros)
            if (want_b) {
#pragma unroll
                for (int p = NS - 1; p >= 0; --p) {
                    accb[0] = mfma16<SP>(gfr[0][p], ones, accb[0]);
                    if (has1) accb[1] = mfma16<SP>(gfr[1][p], ones, accb[1]);
                }
            }
            const char* xrow = s_x + li * W5_PLANE + r * W5_ROWB + 16 * kq;
#pragma unroll
            for (int t = 0; t < C5_T; ++t) {
                const int ky = t / C5_K, kx = t % C5_K;
                u32x4 xfr[NS];
#pragma unroll
                for (int p = 0; p < NS; ++p) __builtin_memcpy(&xfr[p], xrow + p * W5_PIECE + ky * W5_ROWB + kx * 2, 16);
#define BNERV_W5_PROD(pa, pb) acc[0][t] = mfma16<SP>(gfr[0][pa], xfr[pb], acc[0][t]); if (has1) acc[1][t] = mfma16<SP>(gfr[1][pa], xfr[pb], acc[1][t]);
                if constexpr (NS == 3) {
                    BNERV_W5_PROD(2, 0)
                    BNERV_W5_PROD(0, 2)
                    BNERV_W5_PROD(1, 1)
                }
                BNERV_W5_PROD(1, 0)
                BNERV_W5_PROD(0, 1)
                BNERV_W5_PROD(0, 0)
#undef BNERV_W5_PROD
            }
        }
    }

    // ---- slab: lane holds cin = cic * 16 + li, couts co_t0 + 16 n + 4 kq + i
    const int ci = cic * 16 + li;
    float* __restrict__ sw = wa.slab + (size_t)sl * C5_T * Cout * Cin;
    float* __restrict__ sb = wa.slab + (size_t)wa.nslab * C5_T * Cout * Cin + (size_t)sl * Cout;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co_t0 + 16 * n + 4 * kq + i;
            if (co >= Cout) continue;
            if (ci < Cin) {
#pragma unroll
                for (int t = 0; t < C5_T; ++t) sw[((size_t)t * Cout + co) * Cin + ci] = acc[n][t][i];
            }
            if (want_b && li == 0) sb[co] = accb[n][i];
        }
    }
}

// dw[co][ci][t] = sum_sl slab[sl][t][co][ci];  db[co] = sum_sl slabb[sl][co]   (fixed order)
__global__ __launch_bounds__(256) void wgrad5_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw, float* __restrict__ db,
                                                            const int Cin, const int Cout, const int nslab) {
    const int nw = C5_T * Cout * Cin;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < nw) {
        const int t = idx / (Cout * Cin), rem = idx - t * (Cout * Cin);       // slab order: consecutive threads read consecutive addresses
        const int co = rem / Cin, ci = rem - co * Cin;
        float s = 0.f;
        for (int k = 0; k < nslab; ++k) s += slab[(size_t)k * nw + idx];
        dw[((size_t)co * Cin + ci) * C5_T + t] = s;
    } else if (db && idx < nw + Cout) {
        const int co = idx - nw;
        const float* sb = slab + (size_t)nslab * nw;
        float s = 0.f;
        for (int k = 0; k < nslab; ++k) s += sb[(size_t)k * Cout + co];
        db[co] = s;
    }
}

static int w5_nslab(int B, int Cin, int Cout, int H, int W) {
    const int tiles = B * cdiv(H, C5_TH) * cdiv(W, C5_TW);
    const int groups = cdiv(Cin, 16) * cdiv(Cout, W5_CG);
    int n = cdiv(512, groups);
    if (n > tiles) n = tiles;
    if (n > 128) n = 128;
    return n < 1 ? 1 : n;
}

static size_t c5_frag_slots(int Cin, int Cout, int NS) { return (size_t)cdiv(Cin, 16) * cdiv(Cout, 16) * C5_STEPS * NS * 64; }

template <int SP>
static int conv5_launch(hipStream_t st, const C5Args& ka, u32x4* frag) {
    constexpr int NS = Split<SP>::NS;
    const bnerv_conv_desc& d = ka.d;
    const int nprep = ka.nchunk * ka.ntile * C5_STEPS * 64;
    hipLaunchKernelGGL(conv5_wprep_kernel<SP>, dim3(cdiv(nprep, 256)), dim3(256), 0, st, d.w, frag, d.Cin, d.Cout, d.wCi, d.transposed, ka.nchunk, ka.ntile);
    BNERV_LAUNCH_CHECK("conv5_wprep");
    const size_t grid = (size_t)d.B * ka.tiles_y * ka.tiles_x * ka.ngroup;
    hipLaunchKernelGGL(conv5_kernel<SP>, dim3((unsigned)grid), dim3(256), NS * C5_PIECE, st, ka);
    BNERV_LAUNCH_CHECK("conv5");
    return BNERV_OK;
}

static int conv5_validate(const bnerv_conv_desc* d) {
    BNERV_REQUIRE(d, "conv5_igemm: null descriptor");
    BNERV_REQUIRE(d->k == 5, "conv5_igemm: k must be 5 (got %d)", d->k);
    BNERV_REQUIRE(d->x && d->w && d->out, "conv5_igemm: null x / w / out");
    BNERV_REQUIRE(d->B > 0 && d->Cin > 0 && d->Cout > 0 && d->H > 0 && d->W > 0, "conv5_igemm: bad shape B=%d Cin=%d Cout=%d H=%d W=%d", d->B, d->Cin, d->Cout, d->H, d->W);
    BNERV_REQUIRE((size_t)d->Cin * d->H * d->W < (1ull << 31) && (size_t)d->Cout * d->H * d->W < (1ull << 31), "conv5_igemm: sample too large");
    BNERV_REQUIRE(d->in_mode == BNERV_IN_PLAIN || d->in_mode == BNERV_IN_UNSHUFFLE, "conv5_igemm: in_mode %d (IN_PLAIN / IN_UNSHUFFLE)", d->in_mode);
    BNERV_REQUIRE(d->ep_mode == BNERV_EP_BIAS || d->ep_mode == BNERV_EP_BIAS_GELU || d->ep_mode == BNERV_EP_PLAIN,
                  "conv5_igemm: ep_mode %d (EP_BIAS / EP_BIAS_GELU / EP_PLAIN)", d->ep_mode);
    BNERV_REQUIRE(d->out_s == 1 || d->out_s == 2, "conv5_igemm: out_s must be 1 or 2 (got %d)", d->out_s);
    BNERV_REQUIRE(d->out_s == 1 || d->Cout % 4 == 0, "conv5_igemm: Cout=%d not divisible by out_s^2", d->Cout);
    const int in_s = d->in_mode == BNERV_IN_UNSHUFFLE ? d->in_s : 1;
    BNERV_REQUIRE(in_s == 1 || in_s == 2, "conv5_igemm: in_s must be 1 or 2 (got %d)", in_s);
    BNERV_REQUIRE(d->Cin % (in_s * in_s) == 0, "conv5_igemm: Cin=%d not divisible by in_s^2", d->Cin);
    if (d->transposed) BNERV_REQUIRE(d->wCi == d->Cout && d->wCo == d->Cin, "conv5_igemm: transposed weight shape [%d,%d] vs Cin=%d Cout=%d", d->wCo, d->wCi, d->Cin, d->Cout);
    else BNERV_REQUIRE(d->wCo == d->Cout && d->wCi == d->Cin, "conv5_igemm: weight shape [%d,%d] vs Cout=%d Cin=%d", d->wCo, d->wCi, d->Cout, d->Cin);
    if (d->out_s == 2) BNERV_REQUIRE((reinterpret_cast<uintptr_t>(d->out) & 7) == 0 && (reinterpret_cast<uintptr_t>(d->out2) & 7) == 0, "conv5_igemm: out and out2 must be 8-byte aligned when out_s == 2");
    return BNERV_OK;
}

}  // namespace

extern "C" size_t bnerv_conv5_ws_bytes(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return 0;
    return c5_frag_slots(Cin, Cout, 3) * 16;
}

extern "C" int bnerv_conv5_igemm(void* stream, const bnerv_conv_desc* d, void* ws, size_t ws_bytes) {
    const int rc = conv5_validate(d);
    if (rc) return rc;
    BNERV_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, "conv5_igemm: workspace ws must be a 16-byte aligned device buffer");
    if (ws_bytes < bnerv_conv5_ws_bytes(d->Cin, d->Cout)) return bnerv_set_error(BNERV_E_WS, "conv5_igemm: workspace %zu < %zu bytes", ws_bytes, bnerv_conv5_ws_bytes(d->Cin, d->Cout));
    C5Args ka;
    ka.d = *d;
    ka.wfrag = reinterpret_cast<const u32x4*>(ws);
    ka.tiles_x = cdiv(d->W, C5_TW); ka.tiles_y = cdiv(d->H, C5_TH);
    ka.nchunk = cdiv(d->Cin, 16); ka.ntile = cdiv(d->Cout, 16); ka.ngroup = cdiv(ka.ntile, C5_NTB);
    const size_t grid = (size_t)d->B * ka.tiles_y * ka.tiles_x * ka.ngroup;
    BNERV_REQUIRE(grid < (1ull << 31), "conv5_igemm: grid too large");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return c5_x3() ? conv5_launch<SP_BF16X3>(st, ka, reinterpret_cast<u32x4*>(ws)) : conv5_launch<SP_BF16X6>(st, ka, reinterpret_cast<u32x4*>(ws));
}

extern "C" size_t bnerv_conv5_wgrad_ws_bytes(int B, int Cin, int Cout, int H, int W) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)w5_nslab(B, Cin, Cout, H, W) * ((size_t)C5_T * Cout * Cin + Cout) * sizeof(float);
}

extern "C" int bnerv_conv5_wgrad(void* stream, const bnerv_wgrad_desc* d) {
    BNERV_REQUIRE(d, "conv5_wgrad: null descriptor");
    BNERV_REQUIRE(d->k == 5, "conv5_wgrad: k must be 5 (got %d)", d->k);
    BNERV_REQUIRE(d->x && d->g && d->dw, "conv5_wgrad: null x / g / dw");
    BNERV_REQUIRE(d->B > 0 && d->Cin > 0 && d->Cout > 0 && d->H > 0 && d->W > 0, "conv5_wgrad: bad shape B=%d Cin=%d Cout=%d H=%d W=%d", d->B, d->Cin, d->Cout, d->H, d->W);
    BNERV_REQUIRE((size_t)d->Cin * d->H * d->W < (1ull << 31) && (size_t)d->Cout * d->H * d->W < (1ull << 31) && (size_t)C5_T * d->Cout * d->Cin < (1ull << 30),
                  "conv5_wgrad: layer too large");
    BNERV_REQUIRE(d->in_mode == BNERV_IN_PLAIN, "conv5_wgrad: in_mode %d (IN_PLAIN)", d->in_mode);
    BNERV_REQUIRE(d->g_mode == BNERV_IN_PLAIN || d->g_mode == BNERV_IN_UNSHUFFLE, "conv5_wgrad: g_mode %d (IN_PLAIN / IN_UNSHUFFLE)", d->g_mode);
    const int g_s = d->g_mode == BNERV_IN_UNSHUFFLE ? d->g_s : 1;
    BNERV_REQUIRE(g_s == 1 || g_s == 2, "conv5_wgrad: g_s must be 1 or 2 (got %d)", g_s);
    BNERV_REQUIRE(d->Cout % (g_s * g_s) == 0, "conv5_wgrad: Cout=%d not divisible by g_s^2", d->Cout);
    const size_t need = bnerv_conv5_wgrad_ws_bytes(d->B, d->Cin, d->Cout, d->H, d->W);
    BNERV_REQUIRE(d->ws, "conv5_wgrad: null workspace");
    if (d->ws_bytes < need) return bnerv_set_error(BNERV_E_WS, "conv5_wgrad: workspace %zu < %zu bytes", d->ws_bytes, need);
    W5Args wa;
    wa.d = *d;
    wa.slab = reinterpret_cast<float*>(d->ws);
    wa.tiles_x = cdiv(d->W, C5_TW); wa.tiles_y = cdiv(d->H, C5_TH);
    wa.ncic = cdiv(d->Cin, 16); wa.ncog = cdiv(d->Cout, W5_CG);
    wa.nslab = w5_nslab(d->B, d->Cin, d->Cout, d->H, d->W);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)(wa.ncic * wa.ncog * wa.nslab);
    if (c5_x3()) hipLaunchKernelGGL(wgrad5_kernel<SP_BF16X3>, dim3(grid), dim3(256), 2 * W5_PIECE, st, wa);
    else hipLaunchKernelGGL(wgrad5_kernel<SP_BF16X6>, dim3(grid), dim3(256), 3 * W5_PIECE, st, wa);
    BNERV_LAUNCH_CHECK("wgrad5");
    const int n = C5_T * d->Cout * d->Cin + d->Cout;
    hipLaunchKernelGGL(wgrad5_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, wa.slab, d->dw, d->db, d->Cin, d->Cout, wa.nslab);
    BNERV_LAUNCH_CHECK("wgrad5_reduce");
    return BNERV_OK;
}
