// yuv.hip -- raw planar YUV 4:2:0 <-> planar fp32 RGB (boosting_nerv_amd/yuvio.py is the host side and the float64 restatement).
//
// bnerv_yuv420_to_rgb: B frames of a raw clip as they lie in the file (plane Y [H, W], U [H/2, W/2], V [H/2, W/2]; 1 or 2 bytes per sample) ->
// [B, 3, ch, cw] fp32 in [0, 1], the centre crop fused in.  Chroma is up-sampled for MPEG-2 "left" siting on the INTEGER sample values (weights
// 3/4, 1/4 down the rows, 1/2, 1/2 along them: exact in fp32 for codes up to 1023), in source coordinates, so an odd crop offset changes nothing.
// bnerv_rgb_to_yuv420: the inverse for even H and W -- [1 2 1] / 4 along the rows at even x, the mean of the two rows, floor(offset + scale * v + 0.5).
//
// Both are pure streams without LDS.  A thread owns 4 consecutive pixels of a luma row PAIR.  The fp32 side carries 12 of the 13.5 .. 15 bytes a
// pixel moves, so the strip is sized for it: one 16-byte access per row and channel, lane-contiguous (a wave moves 1 KiB per instruction).  The
// sample side of such a strip is 4 or 8 bytes of luma and 2 or 4 bytes of each chroma row, moved as one access each; a 16-sample strip would make
// the luma access 16 bytes and put the fp32 accesses of neighbouring lanes 64 bytes apart.  Of the load's row pair: luma rows 2p + 1 and 2p + 2
// interpolate between the SAME chroma rows p and p + 1 (weights 3/4, 1/4 and 1/4, 3/4), so a thread reads each chroma sample once for two output
// rows.  Every access checks its own address: a pointer, width, stride or crop offset that breaks the alignment of an access sends that access
// (not the launch) to the element-by-element form.
//
// The kernels know nothing of standards: matrix, offsets and scales arrive as one struct of fp32 values computed by the host in float64.
//
// bnerv_yuv420_sse and bnerv_yuv_luma_f32 score packed frames against a window of raw source frames: exact 64-bit sums of
// squared code differences per frame and plane, and the luma plane as fp32 for MS-SSIM.  The same access policy; their shape is described below.
//
// bnerv_yuv420_loss is the training side of that score: the store arithmetic before rounding, minus the source codes, squared
// and averaged per plane, with its exact gradient -- one stream launch of rgb_to_yuv420's shape plus a fixed-order finalize; described below.
//
// bnerv_yuv_luma_pair and bnerv_luma_grad_rgb stand in front of and behind the C = 1 MS-SSIM call of the MS-SSIM-Y term: the
// prediction's luma code before rounding over the peak next to bnerv_yuv_luma_f32's plane, and gY scattered back onto the three RGB planes.
#include "common.h"
#include <stdint.h>

namespace {

constexpr int STRIP = 4, THREADS = 256;

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

// chroma samples row[min(c0 + i, last)], i = 0, 1, 2
template <typename T>
__device__ __forceinline__ void load_chroma3(const T* __restrict__ row, const int c0, const int last, float* v) {
    typedef typename Pack<T>::two W2;
    const T* p = row + c0;
    if (c0 + 1 <= last && (reinterpret_cast<uintptr_t>(p) & (sizeof(W2) - 1)) == 0) {
        unpack2(*reinterpret_cast<const W2*>(p), v);
    } else {
        v[0] = (float)p[0];
        v[1] = (float)row[min(c0 + 1, last)];
    }
    v[2] = (float)row[min(c0 + 2, last)];
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }      // (NaN -> 0)

// grid = (blocks over row pairs x strips, B).  PAR: the parity of every strip's first SOURCE column (left & 1; strips start at multiples of 4)
template <typename T, int PAR>
__global__ __launch_bounds__(THREADS) void yuv420_to_rgb_kernel(const unsigned char* __restrict__ src, const size_t frame_stride, const int H, const int W,
                                                                const int top, const int left, float* __restrict__ out, const int ch, const int cw,
                                                                const int p0, const int npairs, const int nstrips, const bnerv_yuv_coeffs k) {
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t >= npairs * nstrips) return;
    const int pr = t / nstrips, st = t - pr * nstrips;
    const int p = p0 + pr;                                             // luma rows 2p + 1 and 2p + 2, chroma rows p and p + 1 (clamped)
    const int ox0 = st * STRIP, x0 = left + ox0, n = min(STRIP, cw - ox0);
    const int H2 = H >> 1, W2 = W >> 1;
    const T* Y = reinterpret_cast<const T*>(src + (size_t)blockIdx.y * frame_stride);
    const T* U = Y + (size_t)H * W;
    const T* V = U + (size_t)H2 * W2;
    const int ca = max(p, 0), cb = min(p + 1, H2 - 1), c0 = x0 >> 1;
    float ua[3], ub[3], va[3], vb[3];
    load_chroma3(U + (size_t)ca * W2, c0, W2 - 1, ua);
    load_chroma3(U + (size_t)cb * W2, c0, W2 - 1, ub);
    load_chroma3(V + (size_t)ca * W2, c0, W2 - 1, va);
    load_chroma3(V + (size_t)cb * W2, c0, W2 - 1, vb);
    float* const frame = out + (size_t)blockIdx.y * 3 * ch * cw;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = 2 * p + 1 + r;
        if (y < top || y >= top + ch) continue;
        const float wa = r == 0 ? 0.75f : 0.25f, wb = 1.0f - wa;
        float cu[3], cv[3], ys[STRIP];
#pragma unroll
        for (int i = 0; i < 3; ++i) { cu[i] = wa * ua[i] + wb * ub[i]; cv[i] = wa * va[i] + wb * vb[i]; }
        load_luma(Y + (size_t)y * W, x0, n, ys);
        float rgb[3][STRIP];
#pragma unroll
        for (int q = 0; q < STRIP; ++q) {
            const int i = (PAR + q) >> 1;
            const bool odd = (PAR + q) & 1;
            const float u = odd ? 0.5f * (cu[i] + cu[i + 1 > 2 ? 2 : i + 1]) : cu[i];
            const float v = odd ? 0.5f * (cv[i] + cv[i + 1 > 2 ? 2 : i + 1]) : cv[i];
            const float yn = (ys[q] - k.off[0]) * k.scale[0], cbn = (u - k.off[1]) * k.scale[1], crn = (v - k.off[2]) * k.scale[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c][q] = clamp01(k.m[3 * c] * yn + k.m[3 * c + 1] * cbn + k.m[3 * c + 2] * crn);
        }
        const size_t o = (size_t)(y - top) * cw + ox0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = frame + (size_t)c * ch * cw + o;
            if (n == STRIP && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                *reinterpret_cast<f32x4*>(d) = f32x4{rgb[c][0], rgb[c][1], rgb[c][2], rgb[c][3]};
            } else {
#pragma unroll
                for (int q = 0; q < STRIP; ++q)
                    if (q < n) d[q] = rgb[c][q];
            }
        }
    }
}

__device__ __forceinline__ unsigned to_code(float v, float off, float scale, float top) {
    const float c = floorf(off + scale * v + 0.5f);
    return (unsigned)(int)fminf(fmaxf(c, 0.0f), top);
}

template <typename T>
__device__ __forceinline__ void store_samples(T* __restrict__ d, const unsigned* c, const int n, const int whole);
template <>
__device__ __forceinline__ void store_samples<unsigned char>(unsigned char* __restrict__ d, const unsigned* c, const int n, const int whole) {
    if (n == whole && whole == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    } else if (n == whole && whole == 2 && (reinterpret_cast<uintptr_t>(d) & 1) == 0) {
        *reinterpret_cast<uint16_t*>(d) = (uint16_t)(c[0] | (c[1] << 8));
    } else {
        for (int q = 0; q < n; ++q) d[q] = (unsigned char)c[q];
    }
}
template <>
__device__ __forceinline__ void store_samples<unsigned short>(unsigned short* __restrict__ d, const unsigned* c, const int n, const int whole) {
    if (n == whole && whole == 4 && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
        *reinterpret_cast<uint2*>(d) = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
    } else if (n == whole && whole == 2 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = c[0] | (c[1] << 16);
    } else {
        for (int q = 0; q < n; ++q) d[q] = (unsigned short)c[q];
    }
}

// grid = (blocks over row pairs x strips, B).  A thread: luma rows 2j, 2j + 1, columns x0 .. x0 + n (n = 4, or 2 at the end of a row whose width
// is not a multiple of 4) plus the column left of the strip (clamped), which the [1 2 1] filter of the strip's first chroma sample reads.
template <typename T>
__global__ __launch_bounds__(THREADS) void rgb_to_yuv420_kernel(const float* __restrict__ x, const int H, const int W, unsigned char* __restrict__ out,
                                                                const size_t frame_stride, const int nstrips, const bnerv_yuv_coeffs k) {
    const int H2 = H >> 1, W2 = W >> 1;
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t >= H2 * nstrips) return;
    const int j = t / nstrips, st = t - j * nstrips;
    const int x0 = st * STRIP, n = min(STRIP, W - x0), xl = max(x0 - 1, 0);
    const size_t HW = (size_t)H * W;
    const float* const frame = x + (size_t)blockIdx.y * 3 * HW;
    T* const Yp = reinterpret_cast<T*>(out + (size_t)blockIdx.y * frame_stride);
    T* const Up = Yp + HW;
    T* const Vp = Up + (size_t)H2 * W2;
    float cbs[2] = {0.0f, 0.0f}, crs[2] = {0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t o = (size_t)(2 * j + r) * W;
        float c[3][STRIP + 1];                                         // [channel][0: the column left of the strip, 1 + q: column x0 + q]
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float* s = frame + (size_t)a * HW + o;
            c[a][0] = clamp01(s[xl]);
            if (n == STRIP && (reinterpret_cast<uintptr_t>(s + x0) & 15) == 0) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(s + x0);
#pragma unroll
                for (int q = 0; q < STRIP; ++q) c[a][1 + q] = clamp01(v[q]);
            } else {
#pragma unroll
                for (int q = 0; q < STRIP; ++q) c[a][1 + q] = q < n ? clamp01(s[x0 + q]) : 0.0f;
            }
        }
        float cbp[STRIP + 1], crp[STRIP + 1];
        unsigned yc[STRIP];
#pragma unroll
        for (int q = 0; q <= STRIP; ++q) {
            const float R = c[0][q], G = c[1][q], B = c[2][q];
            cbp[q] = k.m[3] * R + k.m[4] * G + k.m[5] * B;
            crp[q] = k.m[6] * R + k.m[7] * G + k.m[8] * B;
            if (q > 0) yc[q - 1] = to_code(k.m[0] * R + k.m[1] * G + k.m[2] * B, k.off[0], k.scale[0], k.maxcode);
        }
        cbs[0] += 0.25f * (cbp[0] + 2.0f * cbp[1] + cbp[2]); cbs[1] += 0.25f * (cbp[2] + 2.0f * cbp[3] + cbp[4]);
        crs[0] += 0.25f * (crp[0] + 2.0f * crp[1] + crp[2]); crs[1] += 0.25f * (crp[2] + 2.0f * crp[3] + crp[4]);
        store_samples<T>(Yp + o + x0, yc, n, STRIP);
    }
    const unsigned uc[2] = {to_code(0.5f * cbs[0], k.off[1], k.scale[1], k.maxcode), to_code(0.5f * cbs[1], k.off[1], k.scale[1], k.maxcode)};
    const unsigned vc[2] = {to_code(0.5f * crs[0], k.off[2], k.scale[2], k.maxcode), to_code(0.5f * crs[1], k.off[2], k.scale[2], k.maxcode)};
    const size_t oc = (size_t)j * W2 + (x0 >> 1);
    store_samples<T>(Up + oc, uc, n >> 1, STRIP / 2);
    store_samples<T>(Vp + oc, vc, n >> 1, STRIP / 2);
}

// ---- scoring: the exact sum of squared code differences per frame and plane, and the luma plane as fp32 ----
//
// yuv420_sse_kernel: grid = (blocks over strips, 3 planes, B).  A strip is 16 bytes of one plane row (16 or 8 samples); a lane takes
// SSE_ITEMS strips, THREADS apart, so a wave's loads are contiguous within a row.  `a` is a packed frame (row pitch = plane width), `b` a
// window of a larger source frame; each side picks the 16-byte load or the element loop by its own address.  Widths: a squared difference is
// below 2^20, a strip's 16 below 2^24, a lane's SSE_ITEMS = 4 strips below 2^26: 32 bits; from the wave sum upward 64 bits.  A wave reduces
// over its lanes with shuffles (no LDS) and lane 0 issues ONE 64-bit atomic add: THREADS / 64 atomics per block and plane.  Integer sums:
// the order of the additions changes no bit.
constexpr int SSE_ITEMS = 4;

__device__ __forceinline__ unsigned sq_diff(unsigned a, unsigned b) { const int d = (int)a - (int)b; return (unsigned)(d * d); }

__device__ __forceinline__ unsigned sse_words(uint32_t wa, uint32_t wb, unsigned char) {
    return sq_diff(wa & 0xffu, wb & 0xffu) + sq_diff((wa >> 8) & 0xffu, (wb >> 8) & 0xffu) + sq_diff((wa >> 16) & 0xffu, (wb >> 16) & 0xffu) +
           sq_diff(wa >> 24, wb >> 24);
}
__device__ __forceinline__ unsigned sse_words(uint32_t wa, uint32_t wb, unsigned short) {
    return sq_diff(wa & 0xffffu, wb & 0xffffu) + sq_diff(wa >> 16, wb >> 16);
}

// n <= 16 / sizeof(T) samples at p as four 32-bit words (samples in memory order, the rest 0): one 16-byte load when the strip is whole and p allows
template <typename T>
__device__ __forceinline__ uint4 load_strip(const T* __restrict__ p, const int n) {
    constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T);
    if (n == S && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < S; ++k)
        if (k < n) w[k / PER] |= (uint32_t)p[k] << (8 * (int)sizeof(T) * (k % PER));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void yuv420_sse_kernel(const unsigned char* __restrict__ a, const size_t a_stride, const unsigned char* __restrict__ b,
                                                             const size_t b_stride, const int H, const int W, const int src_h, const int src_w,
                                                             const int top, const int left, unsigned long long* __restrict__ out) {
    constexpr int S = 16 / (int)sizeof(T);
    const int plane = (int)blockIdx.y, sh = plane ? 1 : 0;
    const int ph = H >> sh, pw = W >> sh, spw = src_w >> sh, ptop = top >> sh, pleft = left >> sh;
    const int nstrips = (pw + S - 1) / S, items = ph * nstrips;
    if ((int)blockIdx.x * (THREADS * SSE_ITEMS) >= items) return;        // (the chroma planes fill a quarter of the luma's blocks)
    const size_t a_off = plane == 0 ? 0 : (size_t)H * W + (plane == 2 ? (size_t)ph * pw : 0);
    const size_t b_off = plane == 0 ? 0 : (size_t)src_h * src_w + (plane == 2 ? (size_t)(src_h >> 1) * spw : 0);
    const T* pa = reinterpret_cast<const T*>(a + (size_t)blockIdx.z * a_stride) + a_off;
    const T* pb = reinterpret_cast<const T*>(b + (size_t)blockIdx.z * b_stride) + b_off + (size_t)ptop * spw + pleft;
    unsigned acc = 0;
#pragma unroll
    for (int k = 0; k < SSE_ITEMS; ++k) {
        const int item = ((int)blockIdx.x * SSE_ITEMS + k) * THREADS + (int)threadIdx.x;
        if (item < items) {
            const int row = item / nstrips, x0 = (item - row * nstrips) * S, n = min(S, pw - x0);
            const uint4 va = load_strip(pa + (size_t)row * pw + x0, n);
            const uint4 vb = load_strip(pb + (size_t)row * spw + x0, n);
            acc += sse_words(va.x, vb.x, T()) + sse_words(va.y, vb.y, T()) + sse_words(va.z, vb.z, T()) + sse_words(va.w, vb.w, T());
        }
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (((int)threadIdx.x & 63) == 0 && sum != 0) atomicAdd(out + (size_t)blockIdx.z * 3 + plane, sum);
}

// grid = (blocks over rows x strips of 4 pixels, B): out[b, 0, y, x] = float(code) / maxcode, the IEEE division
template <typename T>
__global__ __launch_bounds__(THREADS) void yuv_luma_f32_kernel(const unsigned char* __restrict__ src, const size_t frame_stride, const int src_w, const int top,
                                                               const int left, float* __restrict__ out, const int H, const int W, const int nstrips,
                                                               const float maxcode) {
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t >= H * nstrips) return;
    const int y = t / nstrips, x0 = (t - y * nstrips) * STRIP, n = min(STRIP, W - x0);
    const T* Y = reinterpret_cast<const T*>(src + (size_t)blockIdx.y * frame_stride);
    float v[STRIP];
    load_luma(Y + (size_t)(top + y) * src_w, left + x0, n, v);
#pragma unroll
    for (int q = 0; q < STRIP; ++q) v[q] = __fdiv_rn(v[q], maxcode);
    float* d = out + ((size_t)blockIdx.y * H + y) * W + x0;
    if (n == STRIP && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int q = 0; q < STRIP; ++q)
            if (q < n) d[q] = v[q];
    }
}

// ---- the plane loss: rgb_to_yuv420's arithmetic before rounding, minus the source codes, squared; and its exact adjoint ----
//
// yuv420_loss_kernel has rgb_to_yuv420_kernel's shape: grid = (blocks over row pairs x strips, B), a thread owns luma rows 2j, 2j + 1 of columns
// x0 .. x0 + n (n = 4, or 2 at the end of a row), one 16-byte access per channel and row for the prediction and again for the gradient, one access
// per sample row.  The column left of the strip feeds the [1 2 1] filter of the strip's first chroma sample.  The gradient of the strip's last odd
// pixel x0 + 3 also needs the chroma error of sample (x0 + 4) / 2, which belongs to the next thread: it is RECOMPUTED here from the two columns
// right of the strip (they and the next sample's codes are that thread's own loads: L2 hits) instead of exchanged, so one launch gives the sums
// and the gradient and the kernel needs no LDS and no barrier.  No clamp anywhere: the loss is a plain quadratic of the prediction.
//   sums:      every wave writes its three sums of squared errors to ws[b][block * 4 + wave][plane] (wave_sum: shuffles); the finalize adds
//              them lane-strided in fp64 in a fixed order.  No atomics on floats: the same operands give the same bits.
//   gradient:  g = kg[0][c] e_0(y, x) + kg[1][c] t_u(x) + kg[2][c] t_v(x) with t_p(x) = sum_i k(x, i) e_p(j, i) (the taps of section 33) and
//              kg[p][c] = 2 w_p d_p M[p, c] / (B m n_p) (times 1/2 for the row pair on the chroma planes), computed by the host in float64 WITHOUT
//              lambda; written as lambda * g, or added as fma(lambda, g, grad): the accumulating call rounds once more than the writing one.
struct yuvloss_consts {
    float m[9], off[3], d[3], inv_m;       // the store struct's matrix, offsets and denominators; 1 / maxcode
    float kg[9];                           // [plane][channel] gradient constants (above)
    float lambda;
};

template <typename T>
__global__ __launch_bounds__(THREADS) void yuv420_loss_kernel(const float* __restrict__ pred, const int H, const int W, const unsigned char* __restrict__ src,
                                                              const size_t frame_stride, const int n_frames, const int src_h, const int src_w,
                                                              const int top, const int left, const float* __restrict__ frame_sel, const int nstrips,
                                                              float* __restrict__ grad, const int accumulate, float* __restrict__ part,
                                                              const yuvloss_consts k) {
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    float sq[3] = {0.0f, 0.0f, 0.0f};
    if (t < (H >> 1) * nstrips) {                                      // (no early return: every lane takes part in the wave sums below)
        const int b = (int)blockIdx.y;
        int f = b;
        if (frame_sel) f = min(max((int)frame_sel[b], 0), n_frames - 1);
        const int j = t / nstrips, st = t - j * nstrips;
        const int x0 = st * STRIP, n = min(STRIP, W - x0), xl = max(x0 - 1, 0);
        const bool right = x0 + STRIP < W;                             // the next strip exists: W is even, so columns x0 + 4 and x0 + 5 do
        const size_t HW = (size_t)H * W;
        const float* const frame = pred + (size_t)b * 3 * HW;
        const int sw2 = src_w >> 1;
        const T* Y = reinterpret_cast<const T*>(src + (size_t)f * frame_stride);
        const T* U = Y + (size_t)src_h * src_w;
        const T* V = U + (size_t)(src_h >> 1) * sw2;
        const size_t crow = (size_t)((top >> 1) + j) * sw2;
        const int c0 = (left >> 1) + (x0 >> 1), clast = (left >> 1) + (W >> 1) - 1;
        float su[3], sv[3];                                            // codes of chroma samples x0 / 2 + {0, 1, 2} (clamped to the window's last)
        load_chroma3(U + crow, c0, clast, su);
        load_chroma3(V + crow, c0, clast, sv);
        float e0[2][STRIP], cu[3] = {0.0f, 0.0f, 0.0f}, cv[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t o = (size_t)(2 * j + r) * W;
            float c[3][STRIP + 3];                                     // [channel][0: column x0 - 1 (clamped), 1 + q: column x0 + q, q = 0 .. 5]
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float* s = frame + (size_t)a * HW + o;
                c[a][0] = s[xl];
                if (n == STRIP && (reinterpret_cast<uintptr_t>(s + x0) & 15) == 0) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(s + x0);
#pragma unroll
                    for (int q = 0; q < STRIP; ++q) c[a][1 + q] = v[q];
                } else {
#pragma unroll
                    for (int q = 0; q < STRIP; ++q) c[a][1 + q] = q < n ? s[x0 + q] : 0.0f;
                }
                if (right) {
                    const float* h = s + x0 + STRIP;
                    if ((reinterpret_cast<uintptr_t>(h) & 7) == 0) {
                        const f32x2 v = *reinterpret_cast<const f32x2*>(h);
                        c[a][5] = v.x; c[a][6] = v.y;
                    } else {
                        c[a][5] = h[0]; c[a][6] = h[1];
                    }
                } else {
                    c[a][5] = c[a][6] = 0.0f;
                }
            }
            float ys[STRIP], u[STRIP + 3], v[STRIP + 3];
            load_luma(Y + (size_t)(top + 2 * j + r) * src_w, left + x0, n, ys);
#pragma unroll
            for (int q = 0; q < STRIP + 3; ++q) {
                const float R = c[0][q], G = c[1][q], B = c[2][q];
                u[q] = k.m[3] * R + k.m[4] * G + k.m[5] * B;
                v[q] = k.m[6] * R + k.m[7] * G + k.m[8] * B;
                if (q >= 1 && q <= STRIP) {
                    const float e = q - 1 < n ? fmaf(k.d[0], k.m[0] * R + k.m[1] * G + k.m[2] * B, k.off[0] - ys[q - 1]) * k.inv_m : 0.0f;
                    e0[r][q - 1] = e;
                    sq[0] = fmaf(e, e, sq[0]);
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {                              // 4 h_p(2j + r, x0 / 2 + i), summed over the row pair
                cu[i] += u[2 * i] + 2.0f * u[2 * i + 1] + u[2 * i + 2];
                cv[i] += v[2 * i] + 2.0f * v[2 * i + 1] + v[2 * i + 2];
            }
        }
        float eu[3], ev[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const bool have = i == 0 || (i == 1 && n == STRIP) || (i == 2 && right);
            eu[i] = have ? fmaf(k.d[1], 0.125f * cu[i], k.off[1] - su[i]) * k.inv_m : 0.0f;
            ev[i] = have ? fmaf(k.d[2], 0.125f * cv[i], k.off[2] - sv[i]) * k.inv_m : 0.0f;
        }
        sq[1] = eu[0] * eu[0] + eu[1] * eu[1];                         // (sample 2 is the next thread's)
        sq[2] = ev[0] * ev[0] + ev[1] * ev[1];
        if (grad) {
            const float k0 = x0 == 0 ? 0.75f : 0.5f;                   // column 0 is also its own left neighbour
            const float tu[STRIP] = {k0 * eu[0], 0.25f * (eu[0] + eu[1]), 0.5f * eu[1], 0.25f * (eu[1] + eu[2])};
            const float tv[STRIP] = {k0 * ev[0], 0.25f * (ev[0] + ev[1]), 0.5f * ev[1], 0.25f * (ev[1] + ev[2])};
            float* const gframe = grad + (size_t)b * 3 * HW;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float g[STRIP];
#pragma unroll
                    for (int q = 0; q < STRIP; ++q) g[q] = k.kg[a] * e0[r][q] + k.kg[3 + a] * tu[q] + k.kg[6 + a] * tv[q];
                    float* d = gframe + (size_t)a * HW + (size_t)(2 * j + r) * W + x0;
                    if (n == STRIP && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                        f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (accumulate) w = *reinterpret_cast<const f32x4*>(d);
#pragma unroll
                        for (int q = 0; q < STRIP; ++q) w[q] = accumulate ? fmaf(k.lambda, g[q], w[q]) : k.lambda * g[q];
                        *reinterpret_cast<f32x4*>(d) = w;
                    } else {
#pragma unroll
                        for (int q = 0; q < STRIP; ++q)
                            if (q < n) d[q] = accumulate ? fmaf(k.lambda, g[q], d[q]) : k.lambda * g[q];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) sq[p] = wave_sum(sq[p]);
    if (((int)threadIdx.x & 63) == 0) {
        float* o = part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (THREADS / 64) + ((int)threadIdx.x >> 6)) * 3;
        o[0] = sq[0]; o[1] = sq[1]; o[2] = sq[2];
    }
}

// one block: per sample the nparts wave partials of each plane, lane-strided in fp64, then across the four waves; stats, then the batch mean
__global__ __launch_bounds__(THREADS) void yuv420_loss_final_kernel(const float* __restrict__ part, const int B, const int nparts, const double inv_hw,
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

// ---- the MS-SSIM-Y term: the two streams around bnerv_loss_fwd_bwd at C = 1 ----
//
// yuv_luma_pair_kernel: grid = (blocks over rows x strips, B), the stream kernel of section 33.2 without its row pairs.  A thread owns 4 pixels of
// one row: one 16-byte load per prediction channel, one 4- or 8-byte load of the samples, two 16-byte stores.  yp = a0 + a_c P_c with a0 = o_0 / m
// and a_c = d_0 M[0, c] / m formed by the host in float64 (three fmas: the luma code before rounding over the peak, no clamp); ys = code / m with
// the correctly rounded division, the bits of yuv_luma_f32_kernel.  No LDS, no barrier, no atomics.
struct lumapair_consts { float a[3], a0, maxcode; };

__device__ __forceinline__ void load_f32_strip(const float* __restrict__ s, const int n, float* v) {
    if (n == STRIP && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
        for (int q = 0; q < STRIP; ++q) v[q] = w[q];
    } else {
#pragma unroll
        for (int q = 0; q < STRIP; ++q) v[q] = q < n ? s[q] : 0.0f;
    }
}
__device__ __forceinline__ void store_f32_strip(float* __restrict__ d, const int n, const float* v) {
    if (n == STRIP && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int q = 0; q < STRIP; ++q)
            if (q < n) d[q] = v[q];
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void yuv_luma_pair_kernel(const float* __restrict__ pred, const int H, const int W, const unsigned char* __restrict__ src,
                                                                const size_t frame_stride, const int n_frames, const int src_w, const int top,
                                                                const int left, const float* __restrict__ frame_sel, const int nstrips,
                                                                float* __restrict__ yp, float* __restrict__ ys, const lumapair_consts k) {
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t >= H * nstrips) return;
    const int b = (int)blockIdx.y;
    int f = b;
    if (frame_sel) f = min(max((int)frame_sel[b], 0), n_frames - 1);
    const int y = t / nstrips, x0 = (t - y * nstrips) * STRIP, n = min(STRIP, W - x0);
    const size_t HW = (size_t)H * W, o = (size_t)y * W + x0;
    const float* const frame = pred + (size_t)b * 3 * HW + o;
    float c[3][STRIP], s[STRIP], p[STRIP];
#pragma unroll
    for (int a = 0; a < 3; ++a) load_f32_strip(frame + (size_t)a * HW, n, c[a]);
    const T* Y = reinterpret_cast<const T*>(src + (size_t)f * frame_stride);
    load_luma(Y + (size_t)(top + y) * src_w, left + x0, n, s);
#pragma unroll
    for (int q = 0; q < STRIP; ++q) {
        p[q] = fmaf(k.a[0], c[0][q], fmaf(k.a[1], c[1][q], fmaf(k.a[2], c[2][q], k.a0)));
        s[q] = __fdiv_rn(s[q], k.maxcode);
    }
    store_f32_strip(yp + (size_t)b * HW + o, n, p);
    store_f32_strip(ys + (size_t)b * HW + o, n, s);
}

// luma_grad_rgb_kernel: grid = (blocks over strips of a sample's H W values, B).  One 16-byte load of gY, three 16-byte stores (and loads, accumulating):
// grad[b, c] = kk[c] gY or fma(kk[c], gY, grad[b, c]) with kk[c] = lambda k_c.  Thread 0 of the launch: loss = lambda * loss_term, or added by one fma.
__global__ __launch_bounds__(THREADS) void luma_grad_rgb_kernel(const float* __restrict__ gy, const int HW, const int nstrips, const float kk0, const float kk1,
                                                                const float kk2, const float lambda, float* __restrict__ grad, const int accumulate,
                                                                const float* __restrict__ loss_term, float* __restrict__ loss) {
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t == 0 && blockIdx.y == 0) loss[0] = accumulate ? fmaf(lambda, loss_term[0], loss[0]) : lambda * loss_term[0];
    if (t >= nstrips) return;
    const int i0 = t * STRIP, n = min(STRIP, HW - i0);
    const float kk[3] = {kk0, kk1, kk2};
    float g[STRIP];
    load_f32_strip(gy + (size_t)blockIdx.y * HW + i0, n, g);
    float* const frame = grad + (size_t)blockIdx.y * 3 * HW + i0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float* d = frame + (size_t)a * HW;
        float w[STRIP] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (accumulate) load_f32_strip(d, n, w);
#pragma unroll
        for (int q = 0; q < STRIP; ++q) w[q] = accumulate ? fmaf(kk[a], g[q], w[q]) : kk[a] * g[q];
        store_f32_strip(d, n, w);
    }
}

int yuv420_loss_blocks(int H, int W) { return cdiv((H / 2) * cdiv(W, STRIP), THREADS); }

// what every entry point asks of the raw side
int check_raw(const char* what, const void* raw, int bytes_per_sample, int B, size_t frame_stride_bytes, int H, int W) {
    BNERV_REQUIRE(bytes_per_sample == 1 || bytes_per_sample == 2, "%s: bytes_per_sample=%d (1: yuv420p, 2: yuv420p10le)", what, bytes_per_sample);
    BNERV_REQUIRE(B > 0 && B <= 65535, "%s: B=%d", what, B);
    BNERV_REQUIRE(H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu / 4, "%s: H=%d W=%d", what, H, W);
    BNERV_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 needs even dimensions, got %dx%d", what, W, H);
    const size_t frame = (size_t)H * W * 3 / 2 * bytes_per_sample;
    BNERV_REQUIRE(frame_stride_bytes >= frame, "%s: frame_stride_bytes=%zu is smaller than a frame (%zu bytes)", what, frame_stride_bytes, frame);
    BNERV_REQUIRE(bytes_per_sample == 1 || ((reinterpret_cast<uintptr_t>(raw) | frame_stride_bytes) & 1) == 0,
                  "%s: 16-bit samples at an odd address or frame stride", what);
    return BNERV_OK;
}

}  // namespace

extern "C" int bnerv_yuv420_to_rgb(void* stream, const void* src, int bytes_per_sample, int B, size_t frame_stride_bytes, int src_h, int src_w, int top,
                                   int left, float* out, int ch, int cw, const bnerv_yuv_coeffs* coeffs) {
    BNERV_REQUIRE(src && out && coeffs, "yuv420_to_rgb: null args");
    if (const int rc = check_raw("yuv420_to_rgb", src, bytes_per_sample, B, frame_stride_bytes, src_h, src_w)) return rc;
    BNERV_REQUIRE(ch > 0 && cw > 0 && top >= 0 && left >= 0 && top <= src_h - ch && left <= src_w - cw,
                  "yuv420_to_rgb: the %dx%d crop at (top %d, left %d) leaves the %dx%d frame", cw, ch, top, left, src_w, src_h);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "yuv420_to_rgb: out is not 4-byte aligned");
    const int p0 = ((top + 1) >> 1) - 1, npairs = ((top + ch) >> 1) - 1 - p0 + 1, nstrips = cdiv(cw, STRIP);
    const dim3 grid(cdiv(npairs * nstrips, THREADS), B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* raw = static_cast<const unsigned char*>(src);
#define BNERV_YUV_LOAD(T, PAR) \
    hipLaunchKernelGGL((yuv420_to_rgb_kernel<T, PAR>), grid, block, 0, s, raw, frame_stride_bytes, src_h, src_w, top, left, out, ch, cw, p0, npairs, nstrips, *coeffs)
    if (bytes_per_sample == 1) {
        if (left & 1) BNERV_YUV_LOAD(unsigned char, 1); else BNERV_YUV_LOAD(unsigned char, 0);
    } else {
        if (left & 1) BNERV_YUV_LOAD(unsigned short, 1); else BNERV_YUV_LOAD(unsigned short, 0);
    }
#undef BNERV_YUV_LOAD
    BNERV_LAUNCH_CHECK("yuv420_to_rgb");
    return BNERV_OK;
}

extern "C" int bnerv_rgb_to_yuv420(void* stream, const float* x, int B, int H, int W, void* out, int bytes_per_sample, size_t frame_stride_bytes,
                                   const bnerv_yuv_coeffs* coeffs) {
    BNERV_REQUIRE(x && out && coeffs, "rgb_to_yuv420: null args");
    if (const int rc = check_raw("rgb_to_yuv420", out, bytes_per_sample, B, frame_stride_bytes, H, W)) return rc;
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "rgb_to_yuv420: x is not 4-byte aligned");
    const int nstrips = cdiv(W, STRIP);
    const dim3 grid(cdiv((H / 2) * nstrips, THREADS), B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char* raw = static_cast<unsigned char*>(out);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(rgb_to_yuv420_kernel<unsigned char>, grid, block, 0, s, x, H, W, raw, frame_stride_bytes, nstrips, *coeffs);
    else
        hipLaunchKernelGGL(rgb_to_yuv420_kernel<unsigned short>, grid, block, 0, s, x, H, W, raw, frame_stride_bytes, nstrips, *coeffs);
    BNERV_LAUNCH_CHECK("rgb_to_yuv420");
    return BNERV_OK;
}

extern "C" int bnerv_yuv420_sse(void* stream, const void* a, size_t a_stride_bytes, const void* b, size_t b_stride_bytes, int bytes_per_sample, int B,
                                int H, int W, int src_h, int src_w, int top, int left, unsigned long long* out) {
    BNERV_REQUIRE(a && b && out, "yuv420_sse: null args");
    if (const int rc = check_raw("yuv420_sse: a", a, bytes_per_sample, B, a_stride_bytes, H, W)) return rc;
    if (const int rc = check_raw("yuv420_sse: b", b, bytes_per_sample, B, b_stride_bytes, src_h, src_w)) return rc;
    BNERV_REQUIRE(top >= 0 && left >= 0 && top % 2 == 0 && left % 2 == 0, "yuv420_sse: the window offset (top %d, left %d) must be even and not negative",
                  top, left);
    BNERV_REQUIRE(top <= src_h - H && left <= src_w - W, "yuv420_sse: the %dx%d window at (top %d, left %d) leaves the %dx%d frame", W, H, top, left,
                  src_w, src_h);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "yuv420_sse: out is not 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)B * 3 * sizeof(unsigned long long), s);      // (a memset node under capture)
    if (e != hipSuccess) return bnerv_set_error(BNERV_E_LAUNCH, "yuv420_sse: memset: %s", hipGetErrorString(e));
    const int strip = 16 / bytes_per_sample;
    const dim3 grid(cdiv(H * cdiv(W, strip), THREADS * SSE_ITEMS), 3, B), block(THREADS);
    const unsigned char* ra = static_cast<const unsigned char*>(a);
    const unsigned char* rb = static_cast<const unsigned char*>(b);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(yuv420_sse_kernel<unsigned char>, grid, block, 0, s, ra, a_stride_bytes, rb, b_stride_bytes, H, W, src_h, src_w, top, left, out);
    else
        hipLaunchKernelGGL(yuv420_sse_kernel<unsigned short>, grid, block, 0, s, ra, a_stride_bytes, rb, b_stride_bytes, H, W, src_h, src_w, top, left, out);
    BNERV_LAUNCH_CHECK("yuv420_sse");
    return BNERV_OK;
}

extern "C" int bnerv_yuv_luma_f32(void* stream, const void* src, int bytes_per_sample, int B, size_t frame_stride_bytes, int src_h, int src_w, int top,
                                  int left, float* out, int H, int W, float maxcode) {
    BNERV_REQUIRE(src && out, "yuv_luma_f32: null args");
    if (const int rc = check_raw("yuv_luma_f32", src, bytes_per_sample, B, frame_stride_bytes, src_h, src_w)) return rc;
    BNERV_REQUIRE(H > 0 && W > 0 && top >= 0 && left >= 0 && top <= src_h - H && left <= src_w - W,
                  "yuv_luma_f32: the %dx%d window at (top %d, left %d) leaves the %dx%d frame", W, H, top, left, src_w, src_h);
    BNERV_REQUIRE(maxcode >= 1.0f, "yuv_luma_f32: maxcode=%g", (double)maxcode);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "yuv_luma_f32: out is not 4-byte aligned");
    const int nstrips = cdiv(W, STRIP);
    const dim3 grid(cdiv(H * nstrips, THREADS), B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* raw = static_cast<const unsigned char*>(src);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(yuv_luma_f32_kernel<unsigned char>, grid, block, 0, s, raw, frame_stride_bytes, src_w, top, left, out, H, W, nstrips, maxcode);
    else
        hipLaunchKernelGGL(yuv_luma_f32_kernel<unsigned short>, grid, block, 0, s, raw, frame_stride_bytes, src_w, top, left, out, H, W, nstrips, maxcode);
    BNERV_LAUNCH_CHECK("yuv_luma_f32");
    return BNERV_OK;
}

extern "C" size_t bnerv_yuv420_loss_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)H * W > 0x7fffffffu / 4) return 0;
    return (size_t)B * yuv420_loss_blocks(H, W) * (THREADS / 64) * 3 * sizeof(float);
}

extern "C" int bnerv_yuv420_loss(void* stream, const float* pred, int B, int H, int W, const void* src, int bytes_per_sample, size_t frame_stride_bytes,
                                 int n_frames, int src_h, int src_w, int top, int left, const float* frame_sel, const bnerv_yuv_coeffs* coeffs,
                                 const float* weights, float lambda, float* grad, int accumulate, float* loss, float* stats, void* ws, size_t ws_bytes) {
    BNERV_REQUIRE(pred && src && coeffs && weights && loss && stats && ws, "yuv420_loss: null args");
    BNERV_REQUIRE(n_frames > 0, "yuv420_loss: n_frames=%d", n_frames);
    if (const int rc = check_raw("yuv420_loss", src, bytes_per_sample, 1, frame_stride_bytes, src_h, src_w)) return rc;
    BNERV_REQUIRE(B > 0 && B <= 65535 && (frame_sel || B <= n_frames), "yuv420_loss: B=%d samples against %d frames%s", B, n_frames,
                  frame_sel ? "" : " without frame_sel");
    BNERV_REQUIRE(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "yuv420_loss: 4:2:0 needs even dimensions, got %dx%d", W, H);
    BNERV_REQUIRE(top >= 0 && left >= 0 && top % 2 == 0 && left % 2 == 0, "yuv420_loss: the window offset (top %d, left %d) must be even and not negative",
                  top, left);
    BNERV_REQUIRE(top <= src_h - H && left <= src_w - W, "yuv420_loss: the %dx%d window at (top %d, left %d) leaves the %dx%d frame", W, H, top, left,
                  src_w, src_h);
    const double wsum = (double)weights[0] + (double)weights[1] + (double)weights[2];
    BNERV_REQUIRE(weights[0] >= 0.0f && weights[1] >= 0.0f && weights[2] >= 0.0f && wsum > 0.0 && wsum < 1e30,
                  "yuv420_loss: weights (%g, %g, %g) must not be negative and must have a positive finite sum", (double)weights[0], (double)weights[1],
                  (double)weights[2]);
    BNERV_REQUIRE(coeffs->maxcode >= 1.0f, "yuv420_loss: maxcode=%g", (double)coeffs->maxcode);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(loss) |
                    reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(frame_sel)) & 3) == 0,
                  "yuv420_loss: pred, grad, loss, stats, ws and frame_sel must be 4-byte aligned");
    if (ws_bytes < bnerv_yuv420_loss_ws_bytes(B, H, W)) return bnerv_set_error(BNERV_E_WS, "yuv420_loss: workspace too small");
    const int nblocks = yuv420_loss_blocks(H, W), nstrips = cdiv(W, STRIP);
    const double hw = (double)H * W, m = (double)coeffs->maxcode;
    const double w[3] = {weights[0] / wsum, weights[1] / wsum, weights[2] / wsum};
    yuvloss_consts k;
    for (int i = 0; i < 9; ++i) k.m[i] = coeffs->m[i];
    for (int p = 0; p < 3; ++p) {
        k.off[p] = coeffs->off[p];
        k.d[p] = coeffs->scale[p];
        // d L / d a_p per sample: 2 w_p e_p / (B m n_p), n_p = HW or HW / 4; a chroma sample spreads 1/2 to each row of its pair
        const double g = 2.0 * w[p] * (double)coeffs->scale[p] / ((double)B * m * (p ? hw / 4.0 : hw)) * (p ? 0.5 : 1.0);
        for (int c = 0; c < 3; ++c) k.kg[3 * p + c] = (float)(g * (double)coeffs->m[3 * p + c]);
    }
    k.inv_m = (float)(1.0 / m);
    k.lambda = lambda;
    const dim3 grid(nblocks, B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* raw = static_cast<const unsigned char*>(src);
    float* part = static_cast<float*>(ws);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(yuv420_loss_kernel<unsigned char>, grid, block, 0, s, pred, H, W, raw, frame_stride_bytes, n_frames, src_h, src_w, top, left,
                           frame_sel, nstrips, grad, accumulate, part, k);
    else
        hipLaunchKernelGGL(yuv420_loss_kernel<unsigned short>, grid, block, 0, s, pred, H, W, raw, frame_stride_bytes, n_frames, src_h, src_w, top, left,
                           frame_sel, nstrips, grad, accumulate, part, k);
    BNERV_LAUNCH_CHECK("yuv420_loss");
    hipLaunchKernelGGL(yuv420_loss_final_kernel, dim3(1), dim3(THREADS), 0, s, (const float*)part, B, nblocks * (THREADS / 64), 1.0 / hw, w[0], w[1], w[2],
                       lambda, accumulate, loss, stats);
    BNERV_LAUNCH_CHECK("yuv420_loss_final");
    return BNERV_OK;
}

extern "C" int bnerv_yuv_luma_pair(void* stream, const float* pred, int B, int H, int W, const void* src, int bytes_per_sample, size_t frame_stride_bytes,
                                   int n_frames, int src_h, int src_w, int top, int left, const float* frame_sel, const bnerv_yuv_coeffs* coeffs,
                                   float* yp_out, float* ys_out) {
    BNERV_REQUIRE(pred && src && coeffs && yp_out && ys_out, "yuv_luma_pair: null args");
    BNERV_REQUIRE(n_frames > 0, "yuv_luma_pair: n_frames=%d", n_frames);
    if (const int rc = check_raw("yuv_luma_pair", src, bytes_per_sample, 1, frame_stride_bytes, src_h, src_w)) return rc;
    BNERV_REQUIRE(B > 0 && B <= 65535 && (frame_sel || B <= n_frames), "yuv_luma_pair: B=%d samples against %d frames%s", B, n_frames,
                  frame_sel ? "" : " without frame_sel");
    BNERV_REQUIRE(H > 0 && W > 0 && top >= 0 && left >= 0 && top <= src_h - H && left <= src_w - W,
                  "yuv_luma_pair: the %dx%d window at (top %d, left %d) leaves the %dx%d frame", W, H, top, left, src_w, src_h);
    BNERV_REQUIRE(coeffs->maxcode >= 1.0f, "yuv_luma_pair: maxcode=%g", (double)coeffs->maxcode);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(yp_out) | reinterpret_cast<uintptr_t>(ys_out) |
                    reinterpret_cast<uintptr_t>(frame_sel)) & 3) == 0,
                  "yuv_luma_pair: pred, yp_out, ys_out and frame_sel must be 4-byte aligned");
    const double m = (double)coeffs->maxcode;
    lumapair_consts k;
    for (int c = 0; c < 3; ++c) k.a[c] = (float)((double)coeffs->scale[0] * (double)coeffs->m[c] / m);
    k.a0 = (float)((double)coeffs->off[0] / m);
    k.maxcode = coeffs->maxcode;
    const int nstrips = cdiv(W, STRIP);
    const dim3 grid(cdiv(H * nstrips, THREADS), B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* raw = static_cast<const unsigned char*>(src);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(yuv_luma_pair_kernel<unsigned char>, grid, block, 0, s, pred, H, W, raw, frame_stride_bytes, n_frames, src_w, top, left, frame_sel,
                           nstrips, yp_out, ys_out, k);
    else
        hipLaunchKernelGGL(yuv_luma_pair_kernel<unsigned short>, grid, block, 0, s, pred, H, W, raw, frame_stride_bytes, n_frames, src_w, top, left, frame_sel,
                           nstrips, yp_out, ys_out, k);
    BNERV_LAUNCH_CHECK("yuv_luma_pair");
    return BNERV_OK;
}

extern "C" int bnerv_luma_grad_rgb(void* stream, const float* gy, int B, int H, int W, const double* k, float lambda, float* grad, int accumulate,
                                   const float* loss_term, float* loss) {
    BNERV_REQUIRE(k && loss_term && loss && (gy != nullptr) == (grad != nullptr), "luma_grad_rgb: null args");      // (gy and grad both null: the loss word alone)
    BNERV_REQUIRE(B > 0 && B <= 65535, "luma_grad_rgb: B=%d", B);
    BNERV_REQUIRE(H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu / 4, "luma_grad_rgb: H=%d W=%d", H, W);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(loss_term) |
                    reinterpret_cast<uintptr_t>(loss)) & 3) == 0,
                  "luma_grad_rgb: gy, grad, loss_term and loss must be 4-byte aligned");
    const int HW = H * W, nstrips = gy ? cdiv(HW, STRIP) : 0;
    const dim3 grid(gy ? cdiv(nstrips, THREADS) : 1, gy ? B : 1), block(THREADS);
    hipLaunchKernelGGL(luma_grad_rgb_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), gy, HW, nstrips, (float)((double)lambda * k[0]),
                       (float)((double)lambda * k[1]), (float)((double)lambda * k[2]), lambda, grad, accumulate, loss_term, loss);
    BNERV_LAUNCH_CHECK("luma_grad_rgb");
    return BNERV_OK;
}
