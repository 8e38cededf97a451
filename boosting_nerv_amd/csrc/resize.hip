// resize.hip -- the loader's frame resize: separable antialiased bicubic, one axis per launch.
//
// The filter lives on the host (boosting_nerv_amd/resize.py: axis_table): for every output index of an axis a first input index, a tap
// count and normalised fp32 weights.  The kernels only apply a table, and apply it in ONE fixed order so that a numpy fp32 restatement
// gives the same bits (resize.resize_reference):
//     acc = 0.0f;  for j ascending:  acc = fp32(acc + fp32(w_j * x_j))
// -- plain operators under `fp contract(off)` (tap() below): the pragma is what keeps the product and the sum apart (the __fmul_rn /
// __fadd_rn of the HIP headers are inline `x * y` / `x + y` compiled with contraction allowed; interp.hip and codec.hip have the same note).
//
// bnerv_resize_rows  [rows, n_in] -> [rows, n_out].  Neighbouring outputs read inputs `scale` apart, so a lane-per-output global read is
//   strided.  A block instead stages the input span of its RS_STRIP output columns in LDS, one wave per row group: every global read is a
//   contiguous run of a row (16 bytes per lane where the row starts allow it), taps are LDS reads.  A thread keeps one output column for
//   RPT rows, so a weight (read from the TRANSPOSED table: consecutive lanes, consecutive words) is loaded once for RPT taps.
//   LDS reads of neighbouring lanes are `scale` words apart: 2-way bank conflicts at 2x, none at 1x and below.
// bnerv_resize_cols  [planes, n_in, width] -> [planes, n_out, width].  A lane owns a column (or four), a wave an output row: first, count
//   and the weights are uniform over the wave, every tap is one coalesced read of an input row.  An input row is read by about four
//   output rows whatever the scale (support 4 s, stride s); those re-reads hit L2.
// No atomics, no workspace, nothing carried between launches.
#include "common.h"

namespace {
constexpr int RS_STRIP = BNERV_RESIZE_STRIP;       // output columns of a block of the row pass: one wave across
constexpr int RS_WAVES = 4;                        // waves of a block, both passes
constexpr int RS_LDS_BYTES = 48 * 1024;            // what the row pass may stage per block

__device__ __forceinline__ float tap(const float acc, const float w, const float x) {
#pragma clang fp contract(off)
    const float p = w * x;
    return acc + p;
}

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int RPT>
__global__ __launch_bounds__(256) void resize_rows_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ tab,
                                                          const long long rows, const int n_in, const int n_out, const int T, const int pitch,
                                                          const int vec) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int o0 = (int)blockIdx.y * RS_STRIP;
    const int o1 = min(o0 + RS_STRIP, n_out);
    const long long r0 = ((long long)blockIdx.x * RS_WAVES + wv) * RPT;
    // the strip's input span [base, end): first and first + count do not decrease along an axis.  Clamped to the row and to the LDS pitch
    // (the host sized the pitch from the same table; a bad table must not become a wild read)
    int base = clampi(tab[o0], 0, n_in);
    int end = clampi(tab[o1 - 1] + tab[n_out + o1 - 1], base, n_in);
    if (vec) base &= ~3;
    if (end - base > pitch) end = base + pitch;
    float* __restrict__ mine = lds + (size_t)wv * RPT * pitch;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        if (r0 + r >= rows) break;
        const float* __restrict__ src = x + (size_t)(r0 + r) * n_in + base;
        float* __restrict__ dst = mine + r * pitch;
        if (vec) {      // base and n_in are multiples of 4 and every row starts on a 16-byte boundary: the last float4 ends inside the row
            const int n4 = (end - base + 3) >> 2;
            for (int c = lane; c < n4; c += 64) *reinterpret_cast<f32x4*>(dst + 4 * c) = *reinterpret_cast<const f32x4*>(src + 4 * c);
        } else {
            for (int c = lane; c < end - base; c += 64) dst[c] = src[c];
        }
    }
    __syncthreads();
    const int o = o0 + lane;
    if (o >= o1) return;
    int f = tab[o] - base, n = min(tab[n_out + o], T);
    if (f < 0 || n < 0 || f + n > end - base) n = 0;
    const float* __restrict__ wt = reinterpret_cast<const float*>(tab) + (size_t)2 * n_out + (size_t)n_out * T + o;      // weights [T][n_out]
    float acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) acc[r] = 0.0f;
    const float* __restrict__ px = mine + f;
    for (int j = 0; j < n; ++j) {
        const float w = wt[(size_t)j * n_out];
#pragma unroll
        for (int r = 0; r < RPT; ++r) acc[r] = tap(acc[r], w, px[r * pitch + j]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r)
        if (r0 + r < rows) out[(size_t)(r0 + r) * n_out + o] = acc[r];
}

__device__ __forceinline__ float clamp01(const float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__global__ __launch_bounds__(256) void resize_cols_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ tab,
                                                          const int n_in, const int n_out, const int width, const int T, const int vec,
                                                          const int clamp) {
    const int oy = (int)blockIdx.y * RS_WAVES + (int)threadIdx.y;
    if (oy >= n_out) return;
    const int f = clampi(tab[oy], 0, n_in);
    const int n = clampi(min(tab[n_out + oy], T), 0, n_in - f);
    const float* __restrict__ wr = reinterpret_cast<const float*>(tab) + (size_t)2 * n_out + (size_t)oy * T;               // weights [n_out][T]
    const float* __restrict__ src = x + ((size_t)blockIdx.z * n_in + f) * width;
    float* __restrict__ dst = out + ((size_t)blockIdx.z * n_out + oy) * width;
    if (vec) {
        const int i = ((int)blockIdx.x * 64 + (int)threadIdx.x) * 4;
        if (i >= width) return;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)j * width + i);
            const float w = wr[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = tap(acc[k], w, v[k]);
        }
        if (clamp) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = clamp01(acc[k]);
        }
        *reinterpret_cast<f32x4*>(dst + i) = acc;
    } else {
        const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
        if (i >= width) return;
        float acc = 0.0f;
#pragma unroll 4
        for (int j = 0; j < n; ++j) acc = tap(acc, wr[j], src[(size_t)j * width + i]);
        dst[i] = clamp ? clamp01(acc) : acc;
    }
}

int check_axis(const char* who, int n_in, int n_out, int T) {
    BNERV_REQUIRE(n_in > 0 && n_out > 0 && n_in <= (1 << 24) && n_out <= (1 << 24), "%s: n_in=%d n_out=%d (1 .. 2^24 samples on an axis)", who, n_in, n_out);
    BNERV_REQUIRE(T >= 1 && T <= BNERV_RESIZE_MAX_TAPS, "%s: T=%d taps (1 .. %d)", who, T, BNERV_RESIZE_MAX_TAPS);
    return BNERV_OK;
}
}  // namespace

extern "C" int bnerv_resize_rows(void* stream, const float* x, float* out, const void* table_dev, long long rows, int n_in, int n_out, int T, int span) {
    BNERV_REQUIRE(x && out && table_dev, "resize_rows: null args");
    if (int rc = check_axis("resize_rows", n_in, n_out, T)) return rc;
    BNERV_REQUIRE(rows > 0 && rows <= (1LL << 27), "resize_rows: rows=%lld (1 .. 2^27)", rows);      // (blocks x 64 lanes stay below 2^32)
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table_dev)) & 3) == 0,
                  "resize_rows: x, out and the table must be 4-byte aligned");
    BNERV_REQUIRE(span > 0 && span % 4 == 0 && (size_t)span * RS_WAVES * sizeof(float) <= RS_LDS_BYTES,
                  "resize_rows: span=%d floats (a positive multiple of 4; %d rows of it within %d bytes of LDS)", span, RS_WAVES, RS_LDS_BYTES);
    const int strips = cdiv(n_out, RS_STRIP);
    BNERV_REQUIRE(strips <= 65535, "resize_rows: n_out=%d (at most %d output columns)", n_out, 65535 * RS_STRIP);
    // float4 staging: every row starts on a 16-byte boundary
    const int vec = (n_in % 4 == 0) && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int* tab = reinterpret_cast<const int*>(table_dev);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((size_t)span * RS_WAVES * 4 * sizeof(float) <= RS_LDS_BYTES) {
        const long long blocks = (rows + RS_WAVES * 4 - 1) / (RS_WAVES * 4);
        hipLaunchKernelGGL(resize_rows_kernel<4>, dim3((unsigned)blocks, strips), dim3(64, RS_WAVES), (size_t)span * RS_WAVES * 4 * sizeof(float), st,
                           x, out, tab, rows, n_in, n_out, T, span, vec);
    } else {
        const long long blocks = (rows + RS_WAVES - 1) / RS_WAVES;
        hipLaunchKernelGGL(resize_rows_kernel<1>, dim3((unsigned)blocks, strips), dim3(64, RS_WAVES), (size_t)span * RS_WAVES * sizeof(float), st,
                           x, out, tab, rows, n_in, n_out, T, span, vec);
    }
    BNERV_LAUNCH_CHECK("resize_rows");
    return BNERV_OK;
}

extern "C" int bnerv_resize_cols(void* stream, const float* x, float* out, const void* table_dev, int planes, int n_in, int n_out, int width, int T,
                                 int clamp) {
    BNERV_REQUIRE(x && out && table_dev, "resize_cols: null args");
    if (int rc = check_axis("resize_cols", n_in, n_out, T)) return rc;
    BNERV_REQUIRE(planes > 0 && planes <= 65535 && width > 0 && width <= (1 << 24), "resize_cols: planes=%d width=%d (1 <= planes <= 65535, width <= 2^24)",
                  planes, width);
    BNERV_REQUIRE(cdiv(n_out, RS_WAVES) <= 65535, "resize_cols: n_out=%d (at most %d output rows)", n_out, 65535 * RS_WAVES);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table_dev)) & 3) == 0,
                  "resize_cols: x, out and the table must be 4-byte aligned");
    // float4 form: every row of both tensors starts on a 16-byte boundary (width % 4 == 0 and aligned bases); otherwise the scalar form
    const int vec = (width % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(resize_cols_kernel, dim3(cdiv(vec ? width / 4 : width, 64), cdiv(n_out, RS_WAVES), planes), dim3(64, RS_WAVES), 0,
                       reinterpret_cast<hipStream_t>(stream), x, out, reinterpret_cast<const int*>(table_dev), n_in, n_out, width, T, vec, clamp);
    BNERV_LAUNCH_CHECK("resize_cols");
    return BNERV_OK;
}
