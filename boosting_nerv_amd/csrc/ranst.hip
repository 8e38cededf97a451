// ranst.hip -- the kernels of the temporal CEM file (boosting_nerv_amd/tstream.py, codec.encode(..., temporal=True)), in which
// the embedding record of frame t holds either the symbols q_t or the integer differences d_t = q_t - q_{t-1}.
//
// embed_delta          d[t][p] = q[t][p] - q[t-1][p] for t >= 1, and per frame max d, min d, s1 = sum d, s2 = sum d^2 (mod 2^64).  A thread owns
//                      four consecutive p, lanes consecutive quads; every one of the three accesses of a quad (q[t], q[t-1], d[t]) takes the
//                      width its own address allows: 16 bytes, two of 8, or four dwords.  The four statistics are reduced in the wave with
//                      shuffles and leave it as ONE integer atomic each: integer sums commute, so the result does not depend on the order in
//                      which the waves arrive.  min and max travel as order-preserving unsigned keys so that the all-zero state the entry
//                      point sets is their neutral element (no second launch to initialise them).
// embed_chain_dequant  q_t = pred[t] ? q_{t-1} + s_t : s_t,  out[t][p] = float(q_t) * scale[t] + beta[t].  A thread owns one p (consecutive lanes
//                      consecutive p: every access a coalesced dword) and walks t with CHAIN_UNROLL loads in flight ahead of the dependent
//                      adds.  A block serves CHAIN_SEG frames: it starts at the nearest frame at or before its first one that is not predicted
//                      (found from `pred` alone, uniform) and only accumulates up to its own frames, so chains never wait for another block.
//                      The sum is kept in 64 bits; a q_t outside int32 sets bit 0 of the error word and is clamped -- it is a value, never an
//                      address.
#include <limits.h>
#include "common.h"

namespace {

constexpr int THREADS = 256, WAVE = 64, QUAD = 4, DELTA_MAX_BLOCKS_X = 64;
constexpr int CHAIN_UNROLL = BNERV_CHAIN_UNROLL, CHAIN_SEG = BNERV_CHAIN_SEG;
constexpr unsigned SIGN = 0x80000000u;

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// four consecutive dwords at p (4-byte aligned), as wide as the address of p allows
__device__ __forceinline__ int4 load_quad(const int* __restrict__ p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) return *reinterpret_cast<const int4*>(p);
    if ((a & 7u) == 0) {
        const int2 lo = *reinterpret_cast<const int2*>(p), hi = *reinterpret_cast<const int2*>(p + 2);
        return int4{lo.x, lo.y, hi.x, hi.y};
    }
    return int4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void store_quad(int* __restrict__ p, const int4 v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) *reinterpret_cast<int4*>(p) = v;
    else if ((a & 7u) == 0) {
        *reinterpret_cast<int2*>(p) = int2{v.x, v.y};
        *reinterpret_cast<int2*>(p + 2) = int2{v.z, v.w};
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

struct Acc {
    unsigned hi_key, lo_key;      // max over (d ^ SIGN), max over ~(d ^ SIGN): 0 is neutral for both
    long long s1;
    unsigned long long s2;
    __device__ __forceinline__ void add(const int d) {
        const unsigned k = (unsigned)d ^ SIGN;
        hi_key = k > hi_key ? k : hi_key;
        lo_key = ~k > lo_key ? ~k : lo_key;
        s1 += d;
        s2 += (unsigned long long)((long long)d * (long long)d);
    }
};

// grid.x = (N - 1) * bx: block b serves frame t = 1 + b / bx, quads (b % bx) * THREADS + thread, + bx * THREADS, ...
__global__ __launch_bounds__(THREADS) void embed_delta_kernel(const int* __restrict__ q, const size_t q_pitch, int* __restrict__ d, const size_t d_pitch,
                                                              const unsigned P, const unsigned bx, bnerv_delta_stats* __restrict__ stats) {
    const unsigned t = 1u + blockIdx.x / bx, b = blockIdx.x % bx;
    const int* __restrict__ cur = q + (size_t)t * q_pitch;
    const int* __restrict__ prev = cur - q_pitch;
    int* __restrict__ out = d + (size_t)t * d_pitch;
    Acc a = {0u, 0u, 0ll, 0ull};
    const unsigned nq = P / QUAD;
    for (unsigned i = b * THREADS + threadIdx.x; i < nq; i += bx * THREADS) {
        const int4 c = load_quad(cur + (size_t)i * QUAD), p = load_quad(prev + (size_t)i * QUAD);
        const int4 v = {c.x - p.x, c.y - p.y, c.z - p.z, c.w - p.w};       // (int32 wrap for |difference| >= 2^31: the range check on the host sees the wrapped value)
        store_quad(out + (size_t)i * QUAD, v);
        a.add(v.x); a.add(v.y); a.add(v.z); a.add(v.w);
    }
    if (b == 0 && threadIdx.x < P - nq * QUAD) {                          // the at most three elements behind the last quad
        const unsigned i = nq * QUAD + threadIdx.x;
        const int v = cur[i] - prev[i];
        out[i] = v;
        a.add(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned h = (unsigned)__shfl_xor((int)a.hi_key, off, WAVE), l = (unsigned)__shfl_xor((int)a.lo_key, off, WAVE);
        a.hi_key = h > a.hi_key ? h : a.hi_key;
        a.lo_key = l > a.lo_key ? l : a.lo_key;
        a.s1 += __shfl_xor(a.s1, off, WAVE);
        a.s2 += __shfl_xor(a.s2, off, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        bnerv_delta_stats* s = stats + t;
        atomicMax(&s->max_key, a.hi_key);
        atomicMax(&s->min_key_inv, a.lo_key);
        atomicAdd(reinterpret_cast<unsigned long long*>(&s->s1), (unsigned long long)a.s1);      // (two's complement: the signed sum mod 2^64)
        atomicAdd(&s->s2, a.s2);
    }
}

// the product and the sum as two IEEE fp32 operations: dequant1 of csrc/ransw.hip for a record with a beta
__device__ __forceinline__ float dequant_beta(int q, float s, float b) {
#pragma clang fp contract(off)
    const float v = (float)q * s;
    return v + b;
}

// grid: (ceil(P / THREADS), ceil(N / CHAIN_SEG))
__global__ __launch_bounds__(THREADS) void embed_chain_dequant_kernel(const int* __restrict__ sym, const size_t sym_pitch, const unsigned char* __restrict__ pred,
                                                                      const float* __restrict__ scale, const float* __restrict__ beta, float* __restrict__ out,
                                                                      const size_t out_pitch, const unsigned N, const unsigned P, int* __restrict__ err) {
    const unsigned p = blockIdx.x * THREADS + threadIdx.x;
    const unsigned t0 = blockIdx.y * (unsigned)CHAIN_SEG, t1 = N - t0 < (unsigned)CHAIN_SEG ? N : t0 + (unsigned)CHAIN_SEG;       // (t0 < N by the grid)
    unsigned start = t0;                                                  // the head of the chain that frame t0 belongs to (frame 0 heads one whatever pred[0] says)
    while (start > 0 && pred[start] != 0) --start;
    if (p >= P) return;
    long long acc = 0;
    bool bad = false;
    for (unsigned t = start; t < t1; t += CHAIN_UNROLL) {
        int s[CHAIN_UNROLL];
#pragma unroll
        for (int j = 0; j < CHAIN_UNROLL; ++j) s[j] = t + j < t1 ? sym[(size_t)(t + j) * sym_pitch + p] : 0;
#pragma unroll
        for (int j = 0; j < CHAIN_UNROLL; ++j) {
            const unsigned tt = t + j;
            if (tt < t1) {
                acc = (tt > start && pred[tt] != 0) ? acc + s[j] : (long long)s[j];
                if (acc > INT_MAX) { bad = true; acc = INT_MAX; }
                if (acc < INT_MIN) { bad = true; acc = INT_MIN; }
                if (tt >= t0) out[(size_t)tt * out_pitch + p] = dequant_beta((int)acc, scale[tt], beta[tt]);
            }
        }
    }
    if (bad) atomicOr(err, 1);
}

}  // namespace

extern "C" int bnerv_embed_delta(void* stream, const int32_t* q, size_t q_pitch, int n_frames, size_t P, int32_t* d, size_t d_pitch, bnerv_delta_stats* stats) {
    BNERV_REQUIRE(q && d && stats, "embed_delta: null args");
    BNERV_REQUIRE(n_frames > 0 && n_frames <= (1 << 20) && P > 0 && P <= 0x7fffffffu && q_pitch >= P && d_pitch >= P && q_pitch <= 0x7fffffffu && d_pitch <= 0x7fffffffu,
                  "embed_delta: n_frames=%d P=%zu q_pitch=%zu d_pitch=%zu (pitches at least P, all below 2^31, at most 2^20 frames)", n_frames, P, q_pitch, d_pitch);
    BNERV_REQUIRE(aligned(q, 4) && aligned(d, 4) && aligned(stats, 8), "embed_delta: q / d (4 bytes) / stats (8) are not aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, (size_t)n_frames * sizeof(bnerv_delta_stats), st) != hipSuccess) return bnerv_set_error(BNERV_E_LAUNCH, "embed_delta: memset failed");
    if (n_frames == 1) return BNERV_OK;                                   // no frame has a predecessor
    const size_t quads = P / QUAD;
    unsigned bx = (unsigned)((quads + THREADS - 1) / THREADS);
    bx = bx < 1u ? 1u : (bx > (unsigned)DELTA_MAX_BLOCKS_X ? (unsigned)DELTA_MAX_BLOCKS_X : bx);
    hipLaunchKernelGGL(embed_delta_kernel, dim3((unsigned)(n_frames - 1) * bx), dim3(THREADS), 0, st, q, q_pitch, d, d_pitch, (unsigned)P, bx, stats);
    BNERV_LAUNCH_CHECK("embed_delta");
    return BNERV_OK;
}

extern "C" int bnerv_embed_chain_dequant(void* stream, const int32_t* sym, size_t sym_pitch, const unsigned char* pred, const float* scale, const float* beta,
                                         int n_frames, size_t P, float* out, size_t out_pitch, int* err) {
    BNERV_REQUIRE(sym && pred && scale && beta && out && err, "embed_chain_dequant: null args");
    BNERV_REQUIRE(n_frames > 0 && n_frames <= 65535 * BNERV_CHAIN_SEG && P > 0 && P <= 0x7fffffffu && sym_pitch >= P && out_pitch >= P && sym_pitch <= 0x7fffffffu
                  && out_pitch <= 0x7fffffffu, "embed_chain_dequant: n_frames=%d P=%zu sym_pitch=%zu out_pitch=%zu (pitches at least P, all below 2^31)", n_frames, P,
                  sym_pitch, out_pitch);
    BNERV_REQUIRE(aligned(sym, 4) && aligned(scale, 4) && aligned(beta, 4) && aligned(out, 4) && aligned(err, 4),
                  "embed_chain_dequant: sym / scale / beta / out / err are not 4-byte aligned");
    const dim3 grid((unsigned)((P + THREADS - 1) / THREADS), (unsigned)((n_frames + CHAIN_SEG - 1) / CHAIN_SEG));
    hipLaunchKernelGGL(embed_chain_dequant_kernel, grid, dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), sym, sym_pitch, pred, scale, beta, out, out_pitch,
                       (unsigned)n_frames, (unsigned)P, err);
    BNERV_LAUNCH_CHECK("embed_chain_dequant");
    return BNERV_OK;
}
