// hufft.hip -- the kernels of the temporal post-hoc file (boosting_nerv_amd/pstream.py, codec.encode_posthoc(..., temporal=True)),
// in which the embedding of frame t holds either its 8-bit codes q_t or the differences d_t = (q_t - q_{t-1}) mod 256, each kind under a
// Huffman code of its own.  The entropy decode of both strings is huff.hip's kernel with a byte store (bnerv_huff_decode_u8).
//
// embed_delta_u8          d[t][p] = (q[t][p] - q[t-1][p]) mod 256 for t >= 1, and per frame the 256-bin histograms of q_t and of d_t: all the
//                         choice rule (pstream.choose) reads.  A thread owns sixteen consecutive p, lanes consecutive sixteens; every one of its
//                         three accesses (q[t], q[t-1], d[t]) takes the width its own address allows -- 16 bytes, two of 8, four dwords, eight
//                         halves or sixteen bytes -- so a pitch that is no multiple of 16 only changes the width from row to row.  Four codes
//                         are subtracted at a time inside a dword (no borrow crosses a byte).  A block counts into two LDS histograms with
//                         LDS integer atomics and adds its non-zero bins to the frame's with one global integer atomic each: integer sums
//                         commute, so the result does not depend on the order in which the blocks arrive.
// embed_chain_dequant_u8  q_t = pred[t] ? (q_{t-1} + s_t) mod 256 : s_t,  out[t][p] = float(min[s]) + float(scale[s]) * float(q_t[p]) on the
//                         quant_tensor grid of the whole [N, P] tensor.  A thread owns four consecutive p (a dword of codes, added four at
//                         a time; a 16-byte store where the address allows one) and walks t with CHAIN_UNROLL loads in flight ahead of the
//                         dependent adds.  A block serves CHAIN_SEG frames: it starts at the nearest frame at or before its first one that
//                         is not predicted (found from `pred` alone, uniform) and only accumulates up to its own frames, so chains never
//                         wait for another block.  Every value of a byte is a code: there is nothing to flag.
#include "common.h"
#include "huff_rebuild.h"

namespace {

constexpr int THREADS = 256, CHUNK = 16, QUAD = 4, BINS = 256, DELTA_MAX_BLOCKS_X = 64;
constexpr int CHAIN_UNROLL = BNERV_CHAIN_UNROLL, CHAIN_SEG = BNERV_CHAIN_SEG;
constexpr unsigned HIGH = 0x80808080u;
static_assert(THREADS == BINS, "a thread clears and flushes one bin of each histogram");

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// four bytes at a time: (x - y) mod 256 and (x + y) mod 256 in every byte of a dword, no borrow or carry across bytes
__device__ __forceinline__ unsigned sub4(unsigned x, unsigned y) { return ((x | HIGH) - (y & ~HIGH)) ^ ((x ^ ~y) & HIGH); }
__device__ __forceinline__ unsigned add4(unsigned x, unsigned y) { return ((x & ~HIGH) + (y & ~HIGH)) ^ ((x ^ y) & HIGH); }

struct Bytes16 { unsigned w[4]; };        // sixteen consecutive bytes in memory order (little-endian dwords)

// sixteen consecutive bytes at p, as wide as the address of p allows
__device__ __forceinline__ Bytes16 load16(const unsigned char* __restrict__ p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    Bytes16 r;
    if ((a & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
    } else if ((a & 7u) == 0) {
        const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 8);
        r.w[0] = lo.x; r.w[1] = lo.y; r.w[2] = hi.x; r.w[3] = hi.y;
    } else if ((a & 3u) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.w[j] = reinterpret_cast<const unsigned*>(p)[j];
    } else if ((a & 1u) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.w[j] = (unsigned)reinterpret_cast<const unsigned short*>(p)[2 * j] | ((unsigned)reinterpret_cast<const unsigned short*>(p)[2 * j + 1] << 16);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.w[j] = (unsigned)p[4 * j] | ((unsigned)p[4 * j + 1] << 8) | ((unsigned)p[4 * j + 2] << 16) | ((unsigned)p[4 * j + 3] << 24);
    }
    return r;
}
__device__ __forceinline__ void store16(unsigned char* __restrict__ p, const Bytes16& v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) *reinterpret_cast<uint4*>(p) = uint4{v.w[0], v.w[1], v.w[2], v.w[3]};
    else if ((a & 7u) == 0) {
        *reinterpret_cast<uint2*>(p) = uint2{v.w[0], v.w[1]};
        *reinterpret_cast<uint2*>(p + 8) = uint2{v.w[2], v.w[3]};
    } else if ((a & 3u) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) reinterpret_cast<unsigned*>(p)[j] = v.w[j];
    } else if ((a & 1u) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            reinterpret_cast<unsigned short*>(p)[2 * j] = (unsigned short)(v.w[j] & 0xffffu);
            reinterpret_cast<unsigned short*>(p)[2 * j + 1] = (unsigned short)(v.w[j] >> 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = (unsigned char)(v.w[j >> 2] >> (8 * (j & 3)));
    }
}

__device__ __forceinline__ void count16(unsigned* __restrict__ bins, const Bytes16& v) {
#pragma unroll
    for (int j = 0; j < 16; ++j) atomicAdd(&bins[(v.w[j >> 2] >> (8 * (j & 3))) & 255u], 1u);
}

// grid.x = N * bx: block b serves frame t = b / bx, sixteens (b % bx) * THREADS + thread, + bx * THREADS, ...
__global__ __launch_bounds__(THREADS) void embed_delta_u8_kernel(const unsigned char* __restrict__ q, const size_t q_pitch, unsigned char* __restrict__ d,
                                                                 const size_t d_pitch, const unsigned P, const unsigned bx, unsigned* __restrict__ hist) {
    __shared__ unsigned bins[2][BINS];
    const unsigned t = blockIdx.x / bx, b = blockIdx.x % bx;
    bins[0][threadIdx.x] = 0u;
    bins[1][threadIdx.x] = 0u;
    __syncthreads();
    const unsigned char* __restrict__ cur = q + (size_t)t * q_pitch;
    const unsigned nc = P / CHUNK, tail = nc * CHUNK + threadIdx.x;     // (the at most fifteen elements behind the last sixteen: block 0 of the frame)
    if (t == 0) {                                                         // no frame before it: its own histogram only
        for (unsigned i = b * THREADS + threadIdx.x; i < nc; i += bx * THREADS) count16(bins[0], load16(cur + (size_t)i * CHUNK));
        if (b == 0 && tail < P) atomicAdd(&bins[0][cur[tail]], 1u);
    } else {
        const unsigned char* __restrict__ prev = cur - q_pitch;
        unsigned char* __restrict__ out = d + (size_t)t * d_pitch;
        for (unsigned i = b * THREADS + threadIdx.x; i < nc; i += bx * THREADS) {
            const Bytes16 c = load16(cur + (size_t)i * CHUNK), p = load16(prev + (size_t)i * CHUNK);
            Bytes16 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v.w[j] = sub4(c.w[j], p.w[j]);
            store16(out + (size_t)i * CHUNK, v);
            count16(bins[0], c);
            count16(bins[1], v);
        }
        if (b == 0 && tail < P) {
            const unsigned c = cur[tail], v = (c - (unsigned)prev[tail]) & 255u;
            out[tail] = (unsigned char)v;
            atomicAdd(&bins[0][c], 1u);
            atomicAdd(&bins[1][v], 1u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned v = bins[k][threadIdx.x];
        if (v != 0u) atomicAdd(&hist[((size_t)t * 2 + k) * BINS + threadIdx.x], v);
    }
}

// the four codes at p (n of them when the row ends inside the quad), as wide as the address of p allows
__device__ __forceinline__ unsigned load_quad(const unsigned char* __restrict__ p, const unsigned n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (n == (unsigned)QUAD) {
        if ((a & 3u) == 0) return *reinterpret_cast<const unsigned*>(p);
        if ((a & 1u) == 0) return (unsigned)reinterpret_cast<const unsigned short*>(p)[0] | ((unsigned)reinterpret_cast<const unsigned short*>(p)[1] << 16);
        return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    }
    unsigned v = 0u;
    for (unsigned j = 0; j < n; ++j) v |= (unsigned)p[j] << (8u * j);
    return v;
}

// grid: (ceil(ceil(P / QUAD) / THREADS), ceil(N / CHAIN_SEG));  G: the dtype of the grid arrays;  ri = red * inner, 0 for ONE (min, scale) pair
template <typename G>
__global__ __launch_bounds__(THREADS) void embed_chain_dequant_u8_kernel(const unsigned char* __restrict__ sym, const size_t sym_pitch, const unsigned char* __restrict__ pred,
                                                                         const G* __restrict__ mn, const G* __restrict__ sc, const unsigned ri, const unsigned inner,
                                                                         float* __restrict__ out, const size_t out_pitch, const unsigned N, const unsigned P) {
    const unsigned p0 = (blockIdx.x * THREADS + threadIdx.x) * QUAD;
    const unsigned t0 = blockIdx.y * (unsigned)CHAIN_SEG, t1 = N - t0 < (unsigned)CHAIN_SEG ? N : t0 + (unsigned)CHAIN_SEG;       // (t0 < N by the grid)
    unsigned start = t0;                                                  // the head of the chain that frame t0 belongs to (frame 0 heads one whatever pred[0] says)
    while (start > 0 && pred[start] != 0) --start;
    if (p0 >= P) return;
    const unsigned n = P - p0 < (unsigned)QUAD ? P - p0 : (unsigned)QUAD;
    const float mn0 = (float)mn[0], sc0 = (float)sc[0];                   // the pair of a whole-tensor grid
    unsigned acc = 0u;
    for (unsigned t = start; t < t1; t += CHAIN_UNROLL) {
        unsigned s[CHAIN_UNROLL];
#pragma unroll
        for (int j = 0; j < CHAIN_UNROLL; ++j) s[j] = t + j < t1 ? load_quad(sym + (size_t)(t + j) * sym_pitch + p0, n) : 0u;
#pragma unroll
        for (int j = 0; j < CHAIN_UNROLL; ++j) {
            const unsigned tt = t + j;
            if (tt < t1) {
                acc = (tt > start && pred[tt] != 0) ? add4(acc, s[j]) : s[j];
                if (tt >= t0) {
                    float v[QUAD];
#pragma unroll
                    for (int k = 0; k < QUAD; ++k) {
                        const unsigned i = tt * P + p0 + ((unsigned)k < n ? (unsigned)k : n - 1u);      // (below 2^32 by the entry point's check)
                        float m = mn0, c = sc0;
                        if (ri != 0u) {
                            const unsigned g = (i / ri) * inner + i % inner;
                            m = (float)mn[g];
                            c = (float)sc[g];
                        }
                        v[k] = rebuild1(m, c, (acc >> (8 * k)) & 255u);
                    }
                    float* __restrict__ o = out + (size_t)tt * out_pitch + p0;
                    if (n == (unsigned)QUAD && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) *reinterpret_cast<float4*>(o) = float4{v[0], v[1], v[2], v[3]};
                    else {
#pragma unroll
                        for (int k = 0; k < QUAD; ++k)
                            if ((unsigned)k < n) o[k] = v[k];
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" int bnerv_embed_delta_u8(void* stream, const unsigned char* q, size_t q_pitch, int n_frames, size_t P, unsigned char* d, size_t d_pitch, uint32_t* hist) {
    BNERV_REQUIRE(q && d && hist, "embed_delta_u8: null args");
    BNERV_REQUIRE(n_frames > 0 && n_frames <= (1 << 20) && P > 0 && P <= 0x7fffffffu && q_pitch >= P && d_pitch >= P && q_pitch <= 0x7fffffffu && d_pitch <= 0x7fffffffu,
                  "embed_delta_u8: n_frames=%d P=%zu q_pitch=%zu d_pitch=%zu (pitches at least P, all below 2^31, at most 2^20 frames)", n_frames, P, q_pitch, d_pitch);
    BNERV_REQUIRE(aligned(hist, 4), "embed_delta_u8: hist is not 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(hist, 0, (size_t)n_frames * 2 * BINS * sizeof(uint32_t), st) != hipSuccess) return bnerv_set_error(BNERV_E_LAUNCH, "embed_delta_u8: memset failed");
    const size_t chunks = P / CHUNK;
    unsigned bx = (unsigned)((chunks + THREADS - 1) / THREADS);
    bx = bx < 1u ? 1u : (bx > (unsigned)DELTA_MAX_BLOCKS_X ? (unsigned)DELTA_MAX_BLOCKS_X : bx);
    hipLaunchKernelGGL(embed_delta_u8_kernel, dim3((unsigned)n_frames * bx), dim3(THREADS), 0, st, q, q_pitch, d, d_pitch, (unsigned)P, bx, hist);
    BNERV_LAUNCH_CHECK("embed_delta_u8");
    return BNERV_OK;
}

extern "C" int bnerv_embed_chain_dequant_u8(void* stream, const unsigned char* sym, size_t sym_pitch, const unsigned char* pred, const void* min, const void* scale,
                                            int dtype, unsigned red, unsigned inner, int n_frames, size_t P, float* out, size_t out_pitch) {
    BNERV_REQUIRE(sym && pred && min && scale && out, "embed_chain_dequant_u8: null args");
    BNERV_REQUIRE(n_frames > 0 && n_frames <= 65535 * BNERV_CHAIN_SEG && P > 0 && P <= 0x7fffffffu && sym_pitch >= P && out_pitch >= P && sym_pitch <= 0x7fffffffu
                  && out_pitch <= 0x7fffffffu && (unsigned long long)n_frames * P <= 0x7fffffffull,
                  "embed_chain_dequant_u8: n_frames=%d P=%zu sym_pitch=%zu out_pitch=%zu (pitches at least P, all below 2^31, as is n_frames * P)", n_frames, P,
                  sym_pitch, out_pitch);
    const unsigned long long total = (unsigned long long)n_frames * P, ri = (unsigned long long)red * inner;
    BNERV_REQUIRE(red >= 1 && inner >= 1 && ri <= total && total % ri == 0, "embed_chain_dequant_u8: %llu elements do not split into slices of red=%u, inner=%u", total, red, inner);
    BNERV_REQUIRE(dtype == BNERV_HUFF_F32 || dtype == BNERV_HUFF_F16, "embed_chain_dequant_u8: dtype flag %d", dtype);
    const uintptr_t ga = dtype == BNERV_HUFF_F16 ? 2 : 4;
    BNERV_REQUIRE(aligned(out, 4) && aligned(min, ga) && aligned(scale, ga), "embed_chain_dequant_u8: out (4 bytes) / min / scale (their dtype) are not aligned");
    const unsigned quads = (unsigned)((P + QUAD - 1) / QUAD);
    const dim3 grid((quads + THREADS - 1) / THREADS, (unsigned)((n_frames + CHAIN_SEG - 1) / CHAIN_SEG));
    const unsigned one = (ri == total && inner == 1) ? 0u : (unsigned)ri;             // 0: one (min, scale) pair for the whole tensor
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == BNERV_HUFF_F16)
        hipLaunchKernelGGL(embed_chain_dequant_u8_kernel<_Float16>, grid, dim3(THREADS), 0, st, sym, sym_pitch, pred, static_cast<const _Float16*>(min),
                           static_cast<const _Float16*>(scale), one, inner, out, out_pitch, (unsigned)n_frames, (unsigned)P);
    else
        hipLaunchKernelGGL(embed_chain_dequant_u8_kernel<float>, grid, dim3(THREADS), 0, st, sym, sym_pitch, pred, static_cast<const float*>(min),
                           static_cast<const float*>(scale), one, inner, out, out_pitch, (unsigned)n_frames, (unsigned)P);
    BNERV_LAUNCH_CHECK("embed_chain_dequant_u8");
    return BNERV_OK;
}
