// upyuvloss.hip -- the plane loss of DESIGN section 33 taken THROUGH the up-sampler of section 39: a model trained below
// the master's size (--resize_list) is compared against the raw source's planes at the master's size, the number `codec score --upscale`
// reports.  With U the two-pass table filter without its clamp (Q = U P, per channel Q[c] = Wc P[c] Wr^T):
//     L_up(P) = L(U P),      dL_up/dP = Wc^T (dL/dQ) Wr       -- everything is linear up to the quadratic, the gradient is the exact adjoint.
//
// bnerv_yuv420_up_loss_fwd:  bnerv_resize_rows (resize.hip, unchanged: P [B*3, h, w] -> S [B*3, h, W] in the workspace), then
//   up_loss_fwd_kernel     a thread owns what a thread of resize_cols_yuv420_kernel (upyuv.hip) owns -- 4 columns of a luma row PAIR plus the
//                          column left of the strip -- and forms those 2 x 3 x 5 values as that kernel's tap sums (tap() under
//                          `fp contract(off)`, one ascending walk over the union of the two tap ranges): the decoder's up-sampled frame before
//                          its clamp.  It does NOT clamp; it applies yuv420_loss_kernel's arithmetic (yuv.hip) against the source samples
//                          and writes per-wave SSE partials and, when a gradient is wanted, the error planes Ey [B, H, W], Eu, Ev
//                          [B, H/2, W/2], already multiplied by 2 w_p d_p / (B m n_p).  A thread owns its two chroma samples: no halo.
//   up_loss_final_kernel   yuv420_loss_final_kernel: the partials in a fixed order in fp64, stats, the batch mean.
// bnerv_yuv420_up_loss_bwd:
//   up_cols_adj_kernel     a wave per INPUT row i, a lane per column (four with 16-byte accesses where the host found width and addresses fit),
//                          over the adjoint table of h -> H:  Ty[b, i, x] = sum_oy wc Ey[b, oy, x]  at width W,
//                          Tu / Tv[b, i, xc] = sum_oy wc 1/2 E[b, oy >> 1, xc]  at width W/2 (the vertical half of the chroma adjoint commutes
//                          with the horizontal half, so chroma is carried at half width).
//   up_rows_adj_kernel     a block takes 64 input columns and one row per wave; over the output-column span of the strip (adjoint table of
//                          w -> W) it forms  Z_c[ox] = M[0,c] Ty[ox] + sum_p M[p,c] sum_i k(ox, i) T_p[i]  in LDS (section 33.1's taps k), then
//                          every lane gathers its input column:  G[c][x] = sum_j wr_j Z_c[first + j];  lambda * G is written or added.
// Table entries are clamped to the axis and to the LDS pitch wherever they are read.  No float atomics, no inline assembly; nothing is
// allocated or synchronised here.  No [B, 3, H, W] buffer exists on either side.
#include "common.h"
#include <stdint.h>

namespace {

constexpr int STRIP = 4, THREADS = 256;
constexpr int ADJ_STRIP = BNERV_RESIZE_STRIP;      // input columns of a block of the row adjoint: one wave across
constexpr int ADJ_WAVES = 4;
constexpr int ADJ_LDS_BYTES = 48 * 1024;

__device__ __forceinline__ float tap(const float acc, const float w, const float x) {
#pragma clang fp contract(off)
    const float p = w * x;
    return acc + p;
}

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T> struct Pack;                                   // the unsigned word that holds 2 / 4 samples
template <> struct Pack<unsigned char> { typedef uint16_t two; typedef uint32_t four; };
template <> struct Pack<unsigned short> { typedef uint32_t two; typedef uint2 four; };

__device__ __forceinline__ void unpack4(uint32_t w, float* v) {
    v[0] = (float)(w & 0xffu); v[1] = (float)((w >> 8) & 0xffu); v[2] = (float)((w >> 16) & 0xffu); v[3] = (float)(w >> 24);
}
__device__ __forceinline__ void unpack4(uint2 w, float* v) {
    v[0] = (float)(w.x & 0xffffu); v[1] = (float)(w.x >> 16); v[2] = (float)(w.y & 0xffffu); v[3] = (float)(w.y >> 16);
}
__device__ __forceinline__ void unpack2(uint16_t w, float* v) { v[0] = (float)(w & 0xffu); v[1] = (float)(w >> 8); }
__device__ __forceinline__ void unpack2(uint32_t w, float* v) { v[0] = (float)(w & 0xffffu); v[1] = (float)(w >> 16); }

// n <= 4 samples row[i0 .. i0 + n): one access when the strip is whole and its address allows, sample by sample otherwise (the rest: 0)
template <typename T>
__device__ __forceinline__ void load_luma(const T* __restrict__ row, const int i0, const int n, float* v) {
    typedef typename Pack<T>::four W4;
    const T* p = row + i0;
    if (n == STRIP && (reinterpret_cast<uintptr_t>(p) & (sizeof(W4) - 1)) == 0) {
        unpack4(*reinterpret_cast<const W4*>(p), v);
    } else {
#pragma unroll
        for (int k = 0; k < STRIP; ++k) v[k] = k < n ? (float)p[k] : 0.0f;
    }
}

// chroma samples row[c0], row[c0 + 1] (the second only where two == true; else 0)
template <typename T>
__device__ __forceinline__ void load_chroma2(const T* __restrict__ row, const int c0, const bool two, float* v) {
    typedef typename Pack<T>::two W2;
    const T* p = row + c0;
    if (two && (reinterpret_cast<uintptr_t>(p) & (sizeof(W2) - 1)) == 0) {
        unpack2(*reinterpret_cast<const W2*>(p), v);
    } else {
        v[0] = (float)p[0];
        v[1] = two ? (float)p[1] : 0.0f;
    }
}

struct uploss_consts {
    float m[9], off[3], d[3], inv_m;       // the store struct's matrix, offsets and denominators; 1 / maxcode
    float ke[3];                           // 2 w_p d_p / (B m n_p): what an error is multiplied by on its way into the error planes
};

// grid = (blocks over row pairs x strips, B).  A thread: output luma rows 2p, 2p + 1, columns x0 .. x0 + n (n = 4, or 2 at the end of a row whose
// width is not a multiple of 4) plus column max(x0 - 1, 0); chroma samples (p, x0 / 2) and, with n == 4, (p, x0 / 2 + 1).
template <typename T>
__global__ __launch_bounds__(THREADS) void up_loss_fwd_kernel(const float* __restrict__ x, const int* __restrict__ tab, const int n_in, const int H,
                                                              const int W, const int Tt, const unsigned char* __restrict__ src,
                                                              const size_t frame_stride, const int n_frames, const int src_h, const int src_w,
                                                              const int top, const int left, const float* __restrict__ frame_sel, const int nstrips,
                                                              float* __restrict__ Ey, float* __restrict__ Eu, float* __restrict__ Ev,
                                                              float* __restrict__ part, const uploss_consts k) {
    const int H2 = H >> 1, W2 = W >> 1;
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    float sq[3] = {0.0f, 0.0f, 0.0f};
    if (t < H2 * nstrips) {                                            // (no early return: every lane takes part in the wave sums below)
        const int b = (int)blockIdx.y;
        const int p = t / nstrips, st = t - p * nstrips;
        const int x0 = st * STRIP, n = min(STRIP, W - x0), xl = max(x0 - 1, 0);
        // the two tap ranges [f[r], f[r] + cnt[r]) of the input axis, clamped to it, and their weight rows (weights [H][Tt])
        int f[2], cnt[2];
        const float* wr[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int oy = 2 * p + r;
            f[r] = clampi(tab[oy], 0, n_in);
            cnt[r] = clampi(min(tab[H + oy], Tt), 0, n_in - f[r]);
            wr[r] = reinterpret_cast<const float*>(tab) + (size_t)2 * H + (size_t)oy * Tt;
        }
        const int lo = min(f[0], f[1]), hi = max(f[0] + cnt[0], f[1] + cnt[1]);
        const size_t plane = (size_t)n_in * W;
        const float* const frame = x + (size_t)b * 3 * plane;
        float acc[2][3][STRIP + 1];                                    // [row of the pair][channel][0: the column left of the strip, 1 + q: column x0 + q]
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int q = 0; q <= STRIP; ++q) acc[r][a][q] = 0.0f;
        for (int i = lo; i < hi; ++i) {
            float v[3][STRIP + 1];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float* s = frame + (size_t)a * plane + (size_t)i * W;
                v[a][0] = s[xl];
                if (n == STRIP && (reinterpret_cast<uintptr_t>(s + x0) & 15) == 0) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(s + x0);
#pragma unroll
                    for (int q = 0; q < STRIP; ++q) v[a][1 + q] = w4[q];
                } else {
#pragma unroll
                    for (int q = 0; q < STRIP; ++q) v[a][1 + q] = q < n ? s[x0 + q] : 0.0f;
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int j = i - f[r];
                if (j >= 0 && j < cnt[r]) {
                    const float w = wr[r][j];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int q = 0; q <= STRIP; ++q) acc[r][a][q] = tap(acc[r][a][q], w, v[a][q]);
                }
            }
        }
        // from here: yuv420_loss_kernel on acc, NOT clamped
        int fr = b;
        if (frame_sel) fr = min(max((int)frame_sel[b], 0), n_frames - 1);
        const int sw2 = src_w >> 1;
        const T* Y = reinterpret_cast<const T*>(src + (size_t)fr * frame_stride);
        const T* U = Y + (size_t)src_h * src_w;
        const T* V = U + (size_t)(src_h >> 1) * sw2;
        const size_t crow = (size_t)((top >> 1) + p) * sw2;
        const int c0 = (left >> 1) + (x0 >> 1);
        const bool two = n == STRIP;
        float su[2], sv[2];
        load_chroma2(U + crow, c0, two, su);
        load_chroma2(V + crow, c0, two, sv);
        float cu[2] = {0.0f, 0.0f}, cv[2] = {0.0f, 0.0f};
        const size_t HW = (size_t)H * W;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float ys[STRIP], u[STRIP + 1], v[STRIP + 1], e0[STRIP];
            load_luma(Y + (size_t)(top + 2 * p + r) * src_w, left + x0, n, ys);
#pragma unroll
            for (int q = 0; q <= STRIP; ++q) {
                const float R = acc[r][0][q], G = acc[r][1][q], Bl = acc[r][2][q];
                u[q] = k.m[3] * R + k.m[4] * G + k.m[5] * Bl;
                v[q] = k.m[6] * R + k.m[7] * G + k.m[8] * Bl;
                if (q >= 1) {
                    const float e = q - 1 < n ? fmaf(k.d[0], k.m[0] * R + k.m[1] * G + k.m[2] * Bl, k.off[0] - ys[q - 1]) * k.inv_m : 0.0f;
                    e0[q - 1] = e;
                    sq[0] = fmaf(e, e, sq[0]);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {                              // 4 h_p(2p + r, x0 / 2 + i), summed over the row pair
                cu[i] += u[2 * i] + 2.0f * u[2 * i + 1] + u[2 * i + 2];
                cv[i] += v[2 * i] + 2.0f * v[2 * i + 1] + v[2 * i + 2];
            }
            if (Ey) {
                float* d = Ey + (size_t)b * HW + (size_t)(2 * p + r) * W + x0;
                if (n == STRIP && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                    const f32x4 w4 = {k.ke[0] * e0[0], k.ke[0] * e0[1], k.ke[0] * e0[2], k.ke[0] * e0[3]};
                    *reinterpret_cast<f32x4*>(d) = w4;
                } else {
#pragma unroll
                    for (int q = 0; q < STRIP; ++q)
                        if (q < n) d[q] = k.ke[0] * e0[q];
                }
            }
        }
        float eu[2], ev[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool have = i == 0 || two;
            eu[i] = have ? fmaf(k.d[1], 0.125f * cu[i], k.off[1] - su[i]) * k.inv_m : 0.0f;
            ev[i] = have ? fmaf(k.d[2], 0.125f * cv[i], k.off[2] - sv[i]) * k.inv_m : 0.0f;
        }
        sq[1] = eu[0] * eu[0] + eu[1] * eu[1];
        sq[2] = ev[0] * ev[0] + ev[1] * ev[1];
        if (Ey) {
            const size_t oc = (size_t)b * H2 * W2 + (size_t)p * W2 + (x0 >> 1);
            float* du = Eu + oc;
            float* dv = Ev + oc;
            if (two && ((reinterpret_cast<uintptr_t>(du) | reinterpret_cast<uintptr_t>(dv)) & 7) == 0) {
                *reinterpret_cast<f32x2*>(du) = f32x2{k.ke[1] * eu[0], k.ke[1] * eu[1]};
                *reinterpret_cast<f32x2*>(dv) = f32x2{k.ke[2] * ev[0], k.ke[2] * ev[1]};
            } else {
                du[0] = k.ke[1] * eu[0]; dv[0] = k.ke[2] * ev[0];
                if (two) { du[1] = k.ke[1] * eu[1]; dv[1] = k.ke[2] * ev[1]; }
            }
        }
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) sq[pl] = wave_sum(sq[pl]);
    if (((int)threadIdx.x & 63) == 0) {
        float* o = part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (THREADS / 64) + ((int)threadIdx.x >> 6)) * 3;
        o[0] = sq[0]; o[1] = sq[1]; o[2] = sq[2];
    }
}

// one block: per sample the nparts wave partials of each plane, lane-strided in fp64, then across the four waves; stats, then the batch mean
__global__ __launch_bounds__(THREADS) void up_loss_final_kernel(const float* __restrict__ part, const int B, const int nparts, const double inv_hw,
                                                                const double w0, const double w1, const double w2, const float lambda,
                                                                const int accumulate, float* __restrict__ loss, float* __restrict__ stats) {
    __shared__ double red[3][THREADS / 64];
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = (int)threadIdx.x; i < nparts; i += THREADS) {
            const float* p = part + ((size_t)b * nparts + i) * 3;
            s[0] += (double)p[0]; s[1] += (double)p[1]; s[2] += (double)p[2];
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            s[p] = wave_sum_d(s[p]);
            if (((int)threadIdx.x & 63) == 0) red[p][(int)threadIdx.x >> 6] = s[p];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double mse[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) mse[p] = (red[p][0] + red[p][1] + red[p][2] + red[p][3]) * inv_hw * (p ? 4.0 : 1.0);
            const double Lb = w0 * mse[0] + w1 * mse[1] + w2 * mse[2];
            stats[4 * b] = (float)Lb; stats[4 * b + 1] = (float)mse[0]; stats[4 * b + 2] = (float)mse[1]; stats[4 * b + 3] = (float)mse[2];
            total += Lb;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float L = (float)(total / (double)B);
        loss[0] = accumulate ? fmaf(lambda, L, loss[0]) : lambda * L;
    }
}

// grid = (lanes over columns, input rows / ADJ_WAVES, B * 3), block (64, ADJ_WAVES).  Plane z = 3 b + p: p == 0 the luma error plane at width W
// (output row oy is row oy), p = 1, 2 a chroma error plane at width W / 2 (output row oy reads chroma row oy >> 1 at half weight).
// atab: the adjoint table of n_in -> H (n_in entries: the first output row that reads input row i, how many, their weights [n_in][Ta]).
__global__ __launch_bounds__(64 * ADJ_WAVES) void up_cols_adj_kernel(const float* __restrict__ Ey, const float* __restrict__ Eu, const float* __restrict__ Ev,
                                                                     float* __restrict__ Ty, float* __restrict__ Tu, float* __restrict__ Tv,
                                                                     const int* __restrict__ atab, const int n_in, const int H, const int W,
                                                                     const int Ta, const int vec_y, const int vec_c) {
    const int i = (int)blockIdx.y * ADJ_WAVES + (int)threadIdx.y;
    if (i >= n_in) return;
    const int b = (int)blockIdx.z / 3, p = (int)blockIdx.z - 3 * b;
    const int fo = clampi(atab[i], 0, H);
    const int n = clampi(min(atab[n_in + i], Ta), 0, H - fo);
    const float* __restrict__ wa = reinterpret_cast<const float*>(atab) + (size_t)2 * n_in + (size_t)i * Ta;
    const int width = p ? W >> 1 : W, sh = p ? 1 : 0, vec = p ? vec_c : vec_y;
    const float half = p ? 0.5f : 1.0f;
    const float* __restrict__ src = (p == 0 ? Ey : (p == 1 ? Eu : Ev)) + (size_t)b * (H >> sh) * width;
    float* __restrict__ dst = (p == 0 ? Ty : (p == 1 ? Tu : Tv)) + ((size_t)b * n_in + i) * width;
    const int lane = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (vec) {
        const int c = lane * 4;
        if (c >= width) return;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < n; ++j) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)((fo + j) >> sh) * width + c);
            const float w = half * wa[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(w, v[q], acc[q]);
        }
        *reinterpret_cast<f32x4*>(dst + c) = acc;
    } else {
        if (lane >= width) return;
        float acc = 0.0f;
        for (int j = 0; j < n; ++j) acc = fmaf(half * wa[j], src[(size_t)((fo + j) >> sh) * width + lane], acc);
        dst[lane] = acc;
    }
}

// grid = (rows / waves, strips of ADJ_STRIP input columns), block (64, waves); a wave takes row (b, i) of T, LDS 3 * pitch floats per wave.
// atab: the adjoint table of n_in (= w) -> W.  m: the store matrix [plane][channel].
__global__ __launch_bounds__(64 * ADJ_WAVES) void up_rows_adj_kernel(const float* __restrict__ Ty, const float* __restrict__ Tu, const float* __restrict__ Tv,
                                                                     const int* __restrict__ atab, const int rows, const int hh, const int n_in,
                                                                     const int W, const int Ta, const int pitch, const bnerv_yuv_coeffs k,
                                                                     const float lambda, float* __restrict__ grad, const int accumulate) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int row = (int)blockIdx.x * (int)blockDim.y + wv;           // b * hh + i
    const bool live = row < rows;                                     // (no early return: every wave reaches the barrier)
    const int W2 = W >> 1;
    const int x0 = (int)blockIdx.y * ADJ_STRIP, x1 = min(x0 + ADJ_STRIP, n_in);
    // the strip's output span [base, end): first and first + count do not decrease along the axis.  Clamped to the row and to the LDS pitch (the
    // host sized the pitch from the same table; a bad table must not become a wild read)
    const int base = clampi(atab[x0], 0, W) & ~3;
    int end = clampi(atab[x1 - 1] + atab[n_in + x1 - 1], base, W);
    if (end - base > pitch) end = base + pitch;
    float* __restrict__ z = lds + (size_t)wv * 3 * pitch;
    const float* __restrict__ ty = Ty + (size_t)row * W;
    const float* __restrict__ tu = Tu + (size_t)row * W2;
    const float* __restrict__ tv = Tv + (size_t)row * W2;
    for (int o = lane; live && o < end - base; o += 64) {
        const int ox = base + o, ic = ox >> 1;
        float su, sv;
        if (ox & 1) {
            const bool nx = ic + 1 < W2;
            su = 0.25f * (tu[ic] + (nx ? tu[ic + 1] : 0.0f));
            sv = 0.25f * (tv[ic] + (nx ? tv[ic + 1] : 0.0f));
        } else {
            const float k0 = ox == 0 ? 0.75f : 0.5f;                   // column 0 is also its own left neighbour
            su = k0 * tu[ic];
            sv = k0 * tv[ic];
        }
        const float y = ty[ox];
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c * pitch + o] = k.m[c] * y + k.m[3 + c] * su + k.m[6 + c] * sv;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (!live || x >= x1) return;
    int f = atab[x] - base, n = min(atab[n_in + x], Ta);
    if (f < 0 || n < 0 || f + n > end - base) n = 0;
    const float* __restrict__ wt = reinterpret_cast<const float*>(atab) + (size_t)2 * n_in + (size_t)n_in * Ta + x;       // weights [Ta][n_in]
    float g[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < n; ++j) {
        const float w = wt[(size_t)j * n_in];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = fmaf(w, z[c * pitch + f + j], g[c]);
    }
    const int b = row / hh, i = row - b * hh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = grad + (((size_t)b * 3 + c) * hh + i) * n_in + x;
        *d = accumulate ? fmaf(lambda, g[c], *d) : lambda * g[c];
    }
}

inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

int up_loss_blocks(int H, int W) { return cdiv((H / 2) * cdiv(W, STRIP), THREADS); }

// the workspace, in floats: S [B*3, h, W] | Ey [B, H, W] | Eu | Ev [B, H/2, W/2] | Ty [B, h, W] | Tu | Tv [B, h, W/2] | partials; every part
// starts a multiple of 4 floats behind the pointer
struct ws_layout { size_t s, ey, eu, ev, ty, tu, tv, part, total; };

ws_layout layout(int B, int h, int H, int W) {
    ws_layout l;
    const size_t b = (size_t)B, hW = (size_t)h * W, HW = (size_t)H * W;
    size_t at = 0;
    l.s = at; at += round4(b * 3 * hW);
    l.ey = at; at += round4(b * HW);
    l.eu = at; at += round4(b * HW / 4);
    l.ev = at; at += round4(b * HW / 4);
    l.ty = at; at += round4(b * hW);
    l.tu = at; at += round4(b * hW / 2);
    l.tv = at; at += round4(b * hW / 2);
    l.part = at; at += round4(b * up_loss_blocks(H, W) * (THREADS / 64) * 3);
    l.total = at;
    return l;
}

int check_dims(const char* who, int B, int h, int w, int H, int W) {
    BNERV_REQUIRE(B > 0 && B * 3 <= 65535, "%s: B=%d (1 .. 21845)", who, B);
    BNERV_REQUIRE(h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24), "%s: the prediction is %dx%d", who, w, h);
    BNERV_REQUIRE(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 needs even dimensions, the master's size is %dx%d", who, W, H);
    BNERV_REQUIRE((size_t)H * W <= 0x7fffffffu / 4 && (size_t)h * W <= 0x7fffffffu / 4 && (size_t)h * w <= 0x7fffffffu / 4 &&
                      (size_t)B * h <= 0x7fffffffu / 4,
                  "%s: h=%d w=%d H=%d W=%d", who, h, w, H, W);
    return BNERV_OK;
}

}  // namespace

extern "C" size_t bnerv_yuv420_up_loss_ws_bytes(int B, int h, int w, int H, int W) {
    if (B <= 0 || B * 3 > 65535 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || (size_t)H * W > 0x7fffffffu / 4 ||
        (size_t)h * W > 0x7fffffffu / 4)
        return 0;
    return layout(B, h, H, W).total * sizeof(float);
}

extern "C" int bnerv_yuv420_up_loss_fwd(void* stream, const float* pred, int B, int h, int w, int H, int W, const void* table_w_dev, int T_w, int span_w,
                                        const void* table_h_dev, int T_h, const void* src, int bytes_per_sample, size_t frame_stride_bytes,
                                        int n_frames, int src_h, int src_w, int top, int left, const float* frame_sel,
                                        const bnerv_yuv_coeffs* coeffs, const float* weights, float lambda, int need_grad, int accumulate,
                                        float* loss, float* stats, void* ws, size_t ws_bytes) {
    const char* who = "yuv420_up_loss_fwd";
    BNERV_REQUIRE(pred && table_w_dev && table_h_dev && src && coeffs && weights && loss && stats && ws, "%s: null args", who);
    if (const int rc = check_dims(who, B, h, w, H, W)) return rc;
    BNERV_REQUIRE(T_w >= 1 && T_w <= BNERV_RESIZE_MAX_TAPS && T_h >= 1 && T_h <= BNERV_RESIZE_MAX_TAPS, "%s: T_w=%d T_h=%d taps (1 .. %d)", who, T_w, T_h,
                  BNERV_RESIZE_MAX_TAPS);
    BNERV_REQUIRE(n_frames > 0, "%s: n_frames=%d", who, n_frames);
    BNERV_REQUIRE(bytes_per_sample == 1 || bytes_per_sample == 2, "%s: bytes_per_sample=%d (1: yuv420p, 2: yuv420p10le)", who, bytes_per_sample);
    BNERV_REQUIRE(src_h > 0 && src_w > 0 && (size_t)src_h * src_w <= 0x7fffffffu / 4 && src_h % 2 == 0 && src_w % 2 == 0,
                  "%s: 4:2:0 needs a source of even dimensions, got %dx%d", who, src_w, src_h);
    const size_t frame = (size_t)src_h * src_w * 3 / 2 * bytes_per_sample;
    BNERV_REQUIRE(frame_stride_bytes >= frame, "%s: frame_stride_bytes=%zu is smaller than a frame (%zu bytes)", who, frame_stride_bytes, frame);
    BNERV_REQUIRE(bytes_per_sample == 1 || ((reinterpret_cast<uintptr_t>(src) | frame_stride_bytes) & 1) == 0,
                  "%s: 16-bit samples at an odd address or frame stride", who);
    BNERV_REQUIRE(frame_sel || B <= n_frames, "%s: B=%d samples against %d frames without frame_sel", who, B, n_frames);
    BNERV_REQUIRE(top >= 0 && left >= 0 && top % 2 == 0 && left % 2 == 0, "%s: the window offset (top %d, left %d) must be even and not negative", who, top,
                  left);
    BNERV_REQUIRE(top <= src_h - H && left <= src_w - W, "%s: the %dx%d window at (top %d, left %d) leaves the %dx%d frame", who, W, H, top, left, src_w,
                  src_h);
    const double wsum = (double)weights[0] + (double)weights[1] + (double)weights[2];
    BNERV_REQUIRE(weights[0] >= 0.0f && weights[1] >= 0.0f && weights[2] >= 0.0f && wsum > 0.0 && wsum < 1e30,
                  "%s: weights (%g, %g, %g) must not be negative and must have a positive finite sum", who, (double)weights[0], (double)weights[1],
                  (double)weights[2]);
    BNERV_REQUIRE(coeffs->maxcode >= 1.0f, "%s: maxcode=%g", who, (double)coeffs->maxcode);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(ws) |
                    reinterpret_cast<uintptr_t>(frame_sel) | reinterpret_cast<uintptr_t>(table_w_dev) | reinterpret_cast<uintptr_t>(table_h_dev)) & 3) == 0,
                  "%s: pred, loss, stats, ws, frame_sel and the tables must be 4-byte aligned", who);
    const size_t need = bnerv_yuv420_up_loss_ws_bytes(B, h, w, H, W);
    if (need == 0 || ws_bytes < need) return bnerv_set_error(BNERV_E_WS, "yuv420_up_loss_fwd: workspace too small");
    const ws_layout l = layout(B, h, H, W);
    float* const f = static_cast<float*>(ws);
    // P [B*3*h, w] -> S [B*3*h, W] (it validates the rest of its arguments, the LDS span among them, before it launches)
    if (const int rc = bnerv_resize_rows(stream, pred, f + l.s, table_w_dev, (long long)B * 3 * h, w, W, T_w, span_w)) return rc;
    const int nblocks = up_loss_blocks(H, W), nstrips = cdiv(W, STRIP);
    const double hw = (double)H * W, m = (double)coeffs->maxcode;
    const double wn[3] = {weights[0] / wsum, weights[1] / wsum, weights[2] / wsum};
    uploss_consts k;
    for (int i = 0; i < 9; ++i) k.m[i] = coeffs->m[i];
    for (int p = 0; p < 3; ++p) {
        k.off[p] = coeffs->off[p];
        k.d[p] = coeffs->scale[p];
        k.ke[p] = (float)(2.0 * wn[p] * (double)coeffs->scale[p] / ((double)B * m * (p ? hw / 4.0 : hw)));      // d L / d a_p per sample, over e_p
    }
    k.inv_m = (float)(1.0 / m);
    const dim3 grid(nblocks, B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* raw = static_cast<const unsigned char*>(src);
    const int* tab = reinterpret_cast<const int*>(table_h_dev);
    float* const Ey = need_grad ? f + l.ey : nullptr;
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(up_loss_fwd_kernel<unsigned char>, grid, block, 0, s, (const float*)(f + l.s), tab, h, H, W, T_h, raw, frame_stride_bytes, n_frames,
                           src_h, src_w, top, left, frame_sel, nstrips, Ey, f + l.eu, f + l.ev, f + l.part, k);
    else
        hipLaunchKernelGGL(up_loss_fwd_kernel<unsigned short>, grid, block, 0, s, (const float*)(f + l.s), tab, h, H, W, T_h, raw, frame_stride_bytes, n_frames,
                           src_h, src_w, top, left, frame_sel, nstrips, Ey, f + l.eu, f + l.ev, f + l.part, k);
    BNERV_LAUNCH_CHECK("yuv420_up_loss_fwd");
    hipLaunchKernelGGL(up_loss_final_kernel, dim3(1), dim3(THREADS), 0, s, (const float*)(f + l.part), B, nblocks * (THREADS / 64), 1.0 / hw, wn[0], wn[1],
                       wn[2], lambda, accumulate, loss, stats);
    BNERV_LAUNCH_CHECK("yuv420_up_loss_final");
    return BNERV_OK;
}

extern "C" int bnerv_yuv420_up_loss_bwd(void* stream, int B, int h, int w, int H, int W, const void* adj_h_dev, int Ta_h, const void* adj_w_dev, int Ta_w,
                                        int span_a, const bnerv_yuv_coeffs* coeffs, float lambda, float* grad, int accumulate, void* ws,
                                        size_t ws_bytes) {
    const char* who = "yuv420_up_loss_bwd";
    BNERV_REQUIRE(adj_h_dev && adj_w_dev && coeffs && grad && ws, "%s: null args", who);
    if (const int rc = check_dims(who, B, h, w, H, W)) return rc;
    BNERV_REQUIRE(Ta_h >= 1 && Ta_h <= BNERV_RESIZE_MAX_TAPS && Ta_w >= 1 && Ta_w <= BNERV_RESIZE_MAX_TAPS, "%s: Ta_h=%d Ta_w=%d adjoint taps (1 .. %d)", who,
                  Ta_h, Ta_w, BNERV_RESIZE_MAX_TAPS);
    BNERV_REQUIRE(span_a > 0 && span_a % 4 == 0 && (size_t)span_a * 3 * sizeof(float) <= ADJ_LDS_BYTES,
                  "%s: span=%d floats (a positive multiple of 4; three rows of it within %d bytes of LDS)", who, span_a, ADJ_LDS_BYTES);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(adj_h_dev) |
                    reinterpret_cast<uintptr_t>(adj_w_dev)) & 3) == 0,
                  "%s: grad, ws and the tables must be 4-byte aligned", who);
    BNERV_REQUIRE(cdiv(h, ADJ_WAVES) <= 65535 && cdiv(w, ADJ_STRIP) <= 65535, "%s: the prediction is %dx%d", who, w, h);
    const size_t need = bnerv_yuv420_up_loss_ws_bytes(B, h, w, H, W);
    if (need == 0 || ws_bytes < need) return bnerv_set_error(BNERV_E_WS, "yuv420_up_loss_bwd: workspace too small");
    const ws_layout l = layout(B, h, H, W);
    float* const f = static_cast<float*>(ws);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // 16-byte form of a plane: every row of the error plane and of T starts on a 16-byte boundary (the parts of ws start at multiples of 4 floats)
    const int al = (reinterpret_cast<uintptr_t>(ws) & 15) == 0;
    const int vec_y = al && W % 4 == 0, vec_c = al && (W / 2) % 4 == 0 && ((size_t)H / 2 * (W / 2)) % 4 == 0 && ((size_t)h * (W / 2)) % 4 == 0;
    const int lanes = max(vec_y ? W / 4 : W, vec_c ? W / 8 : W / 2);
    hipLaunchKernelGGL(up_cols_adj_kernel, dim3(cdiv(lanes, 64), cdiv(h, ADJ_WAVES), B * 3), dim3(64, ADJ_WAVES), 0, s, (const float*)(f + l.ey),
                       (const float*)(f + l.eu), (const float*)(f + l.ev), f + l.ty, f + l.tu, f + l.tv, reinterpret_cast<const int*>(adj_h_dev), h, H, W, Ta_h,
                       vec_y, vec_c);
    BNERV_LAUNCH_CHECK("yuv420_up_loss_cols_adj");
    const int waves = (size_t)span_a * 3 * ADJ_WAVES * sizeof(float) <= ADJ_LDS_BYTES ? ADJ_WAVES : 1;
    const int rows = B * h;
    hipLaunchKernelGGL(up_rows_adj_kernel, dim3(cdiv(rows, waves), cdiv(w, ADJ_STRIP)), dim3(64, waves), (size_t)span_a * 3 * waves * sizeof(float), s,
                       (const float*)(f + l.ty), (const float*)(f + l.tu), (const float*)(f + l.tv), reinterpret_cast<const int*>(adj_w_dev), rows, h, w, W,
                       Ta_w, span_a, *coeffs, lambda, grad, accumulate);
    BNERV_LAUNCH_CHECK("yuv420_up_loss_rows_adj");
    return BNERV_OK;
}
