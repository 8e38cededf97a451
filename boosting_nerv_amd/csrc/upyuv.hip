// upyuv.hip -- the vertical pass of the frame resize fused with the raw 4:2:0 store: what a decoder that up-samples a
// reduced-resolution model to the master's size runs behind bnerv_resize_rows instead of bnerv_resize_cols + bnerv_rgb_to_yuv420.
//
// bnerv_resize_cols_yuv420: x [B * 3, n_in, W] fp32 (the row pass's output) and the packed axis table of n_in -> H  ->  B raw frames in file
// layout (planes Y [H, W], U, V [H/2, W/2]; 1 or 2 bytes per sample), the bytes bnerv_rgb_to_yuv420 writes for the frame bnerv_resize_cols
// (clamp = 1) would have written -- a frame of 12 H W bytes that is never stored and never read back.
//
// A thread owns what a thread of rgb_to_yuv420_kernel (yuv.hip) owns: 4 columns of a luma row PAIR plus the column left of the strip, which the
// [1 2 1] / 4 filter of the strip's first chroma sample reads.  It does not load those 2 x 3 x 5 values, it forms each as the tap sum of
// resize_cols_kernel (resize.hip) in that kernel's order,  acc = 0.0f;  acc = fp32(acc + fp32(w_j * x_j))  over ascending j, product and sum
// rounded on their own (tap() under `fp contract(off)`).  Output rows 2p and 2p + 1 read almost the same input rows (at 2x: 4 taps each, 5 rows
// together): the thread walks the UNION of the two tap ranges once, in ascending input row, and every loaded value feeds the row(s) whose range
// holds it -- ascending input rows are ascending j for both.  Then clamp01 and, from there, the store kernel's arithmetic word for word.
//
// Access policy of yuv.hip: one 16-byte load per input row and channel where the strip is whole and its address allows, element by element
// otherwise (a misaligned x, W % 4 == 2); samples leave as one packed vector store per row.  Table entries are clamped to the axis as
// resize_cols_kernel clamps them.  No LDS, no atomics, no workspace; nothing is allocated or synchronised in the launch function.
#include "common.h"
#include <stdint.h>

namespace {

constexpr int STRIP = 4, THREADS = 256;

__device__ __forceinline__ float tap(const float acc, const float w, const float x) {
#pragma clang fp contract(off)
    const float p = w * x;
    return acc + p;
}

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }      // (NaN -> 0)

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

// grid = (blocks over row pairs x strips, B).  A thread: output luma rows 2p, 2p + 1, columns x0 .. x0 + n (n = 4, or 2 at the end of a row whose
// width is not a multiple of 4) plus column max(x0 - 1, 0).
template <typename T>
__global__ __launch_bounds__(THREADS) void resize_cols_yuv420_kernel(const float* __restrict__ x, const int* __restrict__ tab, const int n_in, const int H,
                                                                     const int W, const int Tt, unsigned char* __restrict__ out, const size_t frame_stride,
                                                                     const int nstrips, const bnerv_yuv_coeffs k) {
    const int H2 = H >> 1, W2 = W >> 1;
    const int t = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (t >= H2 * nstrips) return;
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
    const float* const frame = x + (size_t)blockIdx.y * 3 * plane;
    float acc[2][3][STRIP + 1];                                        // [row of the pair][channel][0: the column left of the strip, 1 + q: column x0 + q]
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
    // from here: rgb_to_yuv420_kernel on c = clamp01(acc)
    const size_t HW = (size_t)H * W;
    T* const Yp = reinterpret_cast<T*>(out + (size_t)blockIdx.y * frame_stride);
    T* const Up = Yp + HW;
    T* const Vp = Up + (size_t)H2 * W2;
    float cbs[2] = {0.0f, 0.0f}, crs[2] = {0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t o = (size_t)(2 * p + r) * W;
        float cbp[STRIP + 1], crp[STRIP + 1];
        unsigned yc[STRIP];
#pragma unroll
        for (int q = 0; q <= STRIP; ++q) {
            const float R = clamp01(acc[r][0][q]), G = clamp01(acc[r][1][q]), B = clamp01(acc[r][2][q]);
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
    const size_t oc = (size_t)p * W2 + (x0 >> 1);
    store_samples<T>(Up + oc, uc, n >> 1, STRIP / 2);
    store_samples<T>(Vp + oc, vc, n >> 1, STRIP / 2);
}

}  // namespace

extern "C" int bnerv_resize_cols_yuv420(void* stream, const float* x, const void* table_dev, int B, int n_in, int H, int W, int T, void* out,
                                        int bytes_per_sample, size_t frame_stride_bytes, const bnerv_yuv_coeffs* coeffs) {
    const char* who = "resize_cols_yuv420";
    BNERV_REQUIRE(x && table_dev && out && coeffs, "%s: null args", who);
    BNERV_REQUIRE(bytes_per_sample == 1 || bytes_per_sample == 2, "%s: bytes_per_sample=%d (1: yuv420p, 2: yuv420p10le)", who, bytes_per_sample);
    BNERV_REQUIRE(B > 0 && B <= 65535, "%s: B=%d", who, B);
    BNERV_REQUIRE(n_in > 0 && n_in <= (1 << 24), "%s: n_in=%d (1 .. 2^24 rows)", who, n_in);
    BNERV_REQUIRE(H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu / 4 && (size_t)n_in * W <= 0x7fffffffu / 4, "%s: n_in=%d H=%d W=%d", who, n_in, H, W);
    BNERV_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 needs even dimensions, got %dx%d", who, W, H);
    BNERV_REQUIRE(T >= 1 && T <= BNERV_RESIZE_MAX_TAPS, "%s: T=%d taps (1 .. %d)", who, T, BNERV_RESIZE_MAX_TAPS);
    const size_t frame = (size_t)H * W * 3 / 2 * bytes_per_sample;
    BNERV_REQUIRE(frame_stride_bytes >= frame, "%s: frame_stride_bytes=%zu is smaller than a frame (%zu bytes)", who, frame_stride_bytes, frame);
    BNERV_REQUIRE(bytes_per_sample == 1 || ((reinterpret_cast<uintptr_t>(out) | frame_stride_bytes) & 1) == 0,
                  "%s: 16-bit samples at an odd address or frame stride", who);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(table_dev)) & 3) == 0, "%s: x and the table must be 4-byte aligned", who);
    const int nstrips = cdiv(W, STRIP);
    const dim3 grid(cdiv((H / 2) * nstrips, THREADS), B), block(THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int* tab = reinterpret_cast<const int*>(table_dev);
    unsigned char* raw = static_cast<unsigned char*>(out);
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(resize_cols_yuv420_kernel<unsigned char>, grid, block, 0, s, x, tab, n_in, H, W, T, raw, frame_stride_bytes, nstrips, *coeffs);
    else
        hipLaunchKernelGGL(resize_cols_yuv420_kernel<unsigned short>, grid, block, 0, s, x, tab, n_in, H, W, T, raw, frame_stride_bytes, nstrips, *coeffs);
    BNERV_LAUNCH_CHECK("resize_cols_yuv420");
    return BNERV_OK;
}
