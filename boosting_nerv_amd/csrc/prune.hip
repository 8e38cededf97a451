// Global magnitude pruning (include/bnerv.h, "Global magnitude pruning").
//
// kth_abs      most-significant-digit radix select of the k-th smallest key = bits(x) & 0x7fffffff (order-preserving for |x|) over a table of
//              tensors: 4 digits of 8 bits, per digit one histogram launch over the (item, first element) block table and one single-block
//              launch that picks the bin holding the remaining rank.  The select state (prefix, remaining rank, elements below the prefix)
//              stays in device memory between the launches; all of it is integer arithmetic.
//   histogram  a block counts its slice in per-wave private LDS histograms (4 x 256 bins) and adds the non-empty bins to the pass's global
//              histogram: one global atomic per (block, non-empty bin).  Weight magnitudes sit in two or three exponent bins, so on the TOP
//              digit most lanes of a wave hit one LDS address: there the lanes that hold equal digits are counted with ballots and ONE lane
//              adds the count (up to AGG_ROUNDS distinct digits per wave instruction; what is left goes through the plain LDS atomic).
//              The lower digits are mantissa bits of the elements that match the prefix: spread, plain LDS atomics.
// prune_masks  mask = key > tau, x *= mask.        mask_mul / grad_mask_table  x *= mask.
//              A tensor may start at any 4-byte boundary and a mask at any byte: 16-byte accesses over the aligned body of x with the four
//              mask bytes as one dword where the mask address allows, single elements in front of and behind the body.
// Every index that comes from a descriptor is checked against the array it points into before it is used.
#include "common.h"
#include "sidejob.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64, BINS = 256, PASSES = BNERV_KTH_PASSES, SLICE = BNERV_PRUNE_SLICE, AGG_ROUNDS = 4;
constexpr unsigned KEY_MASK = 0x7fffffffu, KEY_INF = 0x7f800000u;
// select state, in dwords behind the PASSES histograms
constexpr int ST_PREFIX = 0, ST_FLAGS = 1, ST_REM = 2 /* u64 */, ST_BELOW = 4 /* u64 */, ST_WORDS = 6;
constexpr size_t WS_WORDS = (size_t)PASSES * BINS + ST_WORDS;

static inline bool aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

struct Span { unsigned head, nq, tail0; };      // [0, head) | nq quads from head | [tail0, n)
__device__ __forceinline__ Span span_of(const float* x, unsigned n) {
    Span s;
    const unsigned h = ((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2;
    s.head = h < n ? h : n;
    s.nq = (n - s.head) >> 2;
    s.tail0 = s.head + s.nq * 4;
    return s;
}
// element `e` (< 6) of the at most three elements in front of and behind the body
__device__ __forceinline__ unsigned edge_index(const Span& s, unsigned e) { return e < s.head ? e : s.tail0 + (e - s.head); }

// the block's slice of its item: false (bit 2 of *flags) for a descriptor that points outside the arrays
__device__ __forceinline__ bool block_slice(const bnerv_prune_item* __restrict__ items, unsigned n_items, const unsigned* __restrict__ blocks,
                                            bool need_mask, unsigned* __restrict__ flags, bnerv_prune_item* it, unsigned* first, unsigned* len) {
    const unsigned item = blocks[2 * blockIdx.x];
    *first = blocks[2 * blockIdx.x + 1];
    bool ok = item < n_items;
    bnerv_prune_item d = {};
    if (ok) d = items[item];
    ok = ok && d.x != nullptr && (!need_mask || d.mask != nullptr) && d.n < 0x80000000u && *first < d.n;
    if (!ok) {
        if (flags && threadIdx.x == 0) atomicOr(flags, 4u);
        return false;
    }
    *it = d;
    *len = d.n - *first < (unsigned)SLICE ? d.n - *first : (unsigned)SLICE;
    return true;
}

// counts `d` in the wave's private histogram; TOP: equal digits of the wave are counted by one lane (the loop runs on wave-uniform state)
template <bool TOP>
__device__ __forceinline__ void count_digit(unsigned* __restrict__ h, unsigned d, bool valid) {
    if (TOP) {
        const unsigned lane = threadIdx.x & 63u;
        unsigned long long todo = __ballot(valid);
        for (int r = 0; r < AGG_ROUNDS && todo; ++r) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned dl = (unsigned)__shfl((int)d, leader, 64);
            const unsigned long long same = __ballot(valid && d == dl);
            if ((int)lane == leader) atomicAdd(&h[dl], (unsigned)__popcll(same));
            todo &= ~same;
            if (d == dl) valid = false;
        }
    }
    if (valid) atomicAdd(&h[d], 1u);
}

template <bool TOP>
__global__ __launch_bounds__(THREADS) void kth_hist_kernel(const bnerv_prune_item* __restrict__ items, const unsigned n_items,
                                                           const unsigned* __restrict__ blocks, unsigned* __restrict__ ws, const int pass) {
    __shared__ unsigned hist[WAVES][BINS];
    unsigned* state = ws + PASSES * BINS;
    bnerv_prune_item it;
    unsigned first, len;
    if (!block_slice(items, n_items, blocks, false, state + ST_FLAGS, &it, &first, &len)) return;
    for (unsigned i = threadIdx.x; i < WAVES * BINS; i += THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    // the digits above this one must equal the prefix found so far (pass 0: there are none, every element counts)
    const unsigned hi_mask = TOP ? 0u : ~((1u << (shift + 8)) - 1u) & KEY_MASK;
    const unsigned prefix = TOP ? 0u : state[ST_PREFIX] & hi_mask;
    unsigned* __restrict__ h = hist[threadIdx.x >> 6];
    const float* __restrict__ x = it.x + first;
    const Span s = span_of(x, len);
    const uint4* __restrict__ x4 = reinterpret_cast<const uint4*>(x + s.head);
    bool nan = false;
    for (unsigned base = 0; base < s.nq; base += THREADS) {            // (uniform trip count: count_digit<true> holds ballots)
        const unsigned i = base + threadIdx.x;
        const bool in = i < s.nq;
        uint4 v = {0u, 0u, 0u, 0u};
        if (in) v = x4[i];
        const unsigned key[4] = {v.x & KEY_MASK, v.y & KEY_MASK, v.z & KEY_MASK, v.w & KEY_MASK};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (TOP) nan = nan || (in && key[j] > KEY_INF);
            count_digit<TOP>(h, (key[j] >> shift) & 0xffu, in && (key[j] & hi_mask) == prefix);
        }
    }
    {
        const unsigned e = threadIdx.x, edge = s.head + (len - s.tail0);       // <= 6 elements
        const bool in = e < edge;
        const unsigned key = in ? __float_as_uint(x[edge_index(s, e)]) & KEY_MASK : 0u;
        if (TOP) nan = nan || (in && key > KEY_INF);
        if (threadIdx.x < 64) count_digit<TOP>(h, (key >> shift) & 0xffu, in && (key & hi_mask) == prefix);
    }
    if (TOP && nan) atomicOr(state + ST_FLAGS, 1u);
    __syncthreads();
    unsigned* out = ws + pass * BINS;
    for (unsigned b = threadIdx.x; b < BINS; b += THREADS) {
        const unsigned c = (hist[0][b] + hist[1][b]) + (hist[2][b] + hist[3][b]);
        if (c) atomicAdd(&out[b], c);
    }
}

// one block: the bin of pass `pass` that holds the remaining rank; the last pass writes the result
__global__ __launch_bounds__(BINS) void kth_pick_kernel(unsigned* __restrict__ ws, const int pass, const unsigned long long k, unsigned* __restrict__ out) {
    __shared__ unsigned wave_tot[BINS / 64];
    __shared__ unsigned s_bin, s_before, s_count;
    unsigned* state = ws + PASSES * BINS;
    const unsigned t = threadIdx.x, lane = t & 63u;
    const unsigned c = ws[pass * BINS + t];
    unsigned incl = c;                                                 // inclusive scan of the 256 counts (a table has fewer than 2^32 elements)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, off, 64);
        if ((int)lane >= off) incl += up;
    }
    if (lane == 63) wave_tot[t >> 6] = incl;
    if (t == 0) { s_bin = BINS; s_before = 0; s_count = 0; }
    __syncthreads();
    unsigned before_wave = 0;
    for (unsigned w = 0; w < (t >> 6); ++w) before_wave += wave_tot[w];
    const unsigned long long rem = pass == 0 ? k : *reinterpret_cast<const unsigned long long*>(state + ST_REM);
    const unsigned long long lo = (unsigned long long)before_wave + (incl - c), hi = lo + c;       // ranks (lo, hi] fall into bin t
    if (rem > lo && rem <= hi) { s_bin = t; s_before = (unsigned)lo; s_count = c; }                  // (at most one thread: the ranges are disjoint)
    __syncthreads();
    if (t == 0) {
        const int shift = 24 - 8 * pass;
        unsigned flags = state[ST_FLAGS];
        unsigned bin = s_bin;
        if (bin >= BINS) { flags |= 2u; bin = BINS - 1; }              // k == 0 or k beyond the element count: flagged, the largest key
        const unsigned prefix = (pass == 0 ? 0u : state[ST_PREFIX]) | (bin << shift);
        const unsigned long long below = (pass == 0 ? 0ull : *reinterpret_cast<const unsigned long long*>(state + ST_BELOW)) + s_before;
        state[ST_PREFIX] = prefix;
        state[ST_FLAGS] = flags;
        *reinterpret_cast<unsigned long long*>(state + ST_REM) = rem - s_before;
        *reinterpret_cast<unsigned long long*>(state + ST_BELOW) = below;
        if (pass == PASSES - 1) {
            out[0] = prefix;
            out[1] = flags;
            *reinterpret_cast<unsigned long long*>(out + 2) = below + s_count;     // elements below tau + elements equal to it
        }
    }
}

// x[i] *= m[i] (BUILD: m[i] = key(x[i]) > tau first) for block bx of gx over n elements
template <bool BUILD>
__device__ __forceinline__ void mask_span(float* __restrict__ x, unsigned char* __restrict__ m, const unsigned n, const unsigned tau,
                                          const unsigned bx, const unsigned gx) {
    const Span s = span_of(x, n);
    f32x4* __restrict__ x4 = reinterpret_cast<f32x4*>(x + s.head);
    unsigned char* __restrict__ mb = m + s.head;
    const bool m4 = (reinterpret_cast<uintptr_t>(mb) & 3u) == 0;       // block-uniform: the four mask bytes of a quad as one dword
    for (unsigned i = bx * THREADS + threadIdx.x; i < s.nq; i += gx * THREADS) {
        f32x4 v = x4[i];
        unsigned char k0, k1, k2, k3;
        if (BUILD) {
            k0 = (__float_as_uint(v[0]) & KEY_MASK) > tau; k1 = (__float_as_uint(v[1]) & KEY_MASK) > tau;
            k2 = (__float_as_uint(v[2]) & KEY_MASK) > tau; k3 = (__float_as_uint(v[3]) & KEY_MASK) > tau;
            if (m4) reinterpret_cast<unsigned*>(mb)[i] = (unsigned)k0 | ((unsigned)k1 << 8) | ((unsigned)k2 << 16) | ((unsigned)k3 << 24);
            else { mb[4 * i] = k0; mb[4 * i + 1] = k1; mb[4 * i + 2] = k2; mb[4 * i + 3] = k3; }
        } else if (m4) {
            const unsigned w = reinterpret_cast<const unsigned*>(mb)[i];
            k0 = w & 0xffu; k1 = (w >> 8) & 0xffu; k2 = (w >> 16) & 0xffu; k3 = w >> 24;
        } else {
            k0 = mb[4 * i]; k1 = mb[4 * i + 1]; k2 = mb[4 * i + 2]; k3 = mb[4 * i + 3];
        }
        v[0] *= (float)k0; v[1] *= (float)k1; v[2] *= (float)k2; v[3] *= (float)k3;
        x4[i] = v;
    }
    if (bx == 0) {
        const unsigned e = threadIdx.x, edge = s.head + (n - s.tail0);
        if (e < edge) {
            const unsigned i = edge_index(s, e);
            const float v = x[i];
            unsigned char k;
            if (BUILD) { k = (__float_as_uint(v) & KEY_MASK) > tau; m[i] = k; }
            else k = m[i];
            x[i] = v * (float)k;
        }
    }
}

template <bool BUILD>
__global__ __launch_bounds__(THREADS) void mask_items_kernel(const bnerv_prune_item* __restrict__ items, const unsigned n_items,
                                                             const unsigned* __restrict__ blocks, const unsigned* __restrict__ tau_dev) {
    bnerv_prune_item it;
    unsigned first, len;
    if (!block_slice(items, n_items, blocks, true, nullptr, &it, &first, &len)) return;
    mask_span<BUILD>(it.x + first, it.mask + first, len, BUILD ? tau_dev[0] : 0u, 0u, 1u);
}

__global__ __launch_bounds__(THREADS) void grad_mask_table_kernel(const bnerv_adan_entry* __restrict__ tab, const int n_tensors,
                                                                  const unsigned char* const* __restrict__ masks) {
    int t = 0;                                                         // the tensor of this block: bisection over bstart, as the optimizer kernels
    for (int hi = n_tensors; hi - t > 1;) {
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= tab[mid].bstart) t = mid; else hi = mid;
    }
    const unsigned char* m = masks[t];
    if (m == nullptr) return;
    const bnerv_adan_entry e = tab[t];
    int gx = (e.n + THREADS * 4 - 1) / (THREADS * 4);
    if (gx > 1024) gx = 1024;
    mask_span<false>(const_cast<float*>(e.g), const_cast<unsigned char*>(m), (unsigned)e.n, 0u, (unsigned)((int)blockIdx.x - e.bstart), (unsigned)gx);
}

int check_table(const char* what, const void* items, int n_items, const void* blocks, size_t n_blocks) {
    BNERV_REQUIRE(items && blocks, "%s: null args", what);
    BNERV_REQUIRE(n_items > 0 && n_blocks > 0 && n_blocks <= 0x7fffffffu, "%s: n_items=%d n_blocks=%zu", what, n_items, n_blocks);
    BNERV_REQUIRE(aligned(items, 8) && aligned(blocks, 4), "%s: items (8 bytes) / blocks (4) are not aligned", what);
    return BNERV_OK;
}

}  // namespace

extern "C" int bnerv_kth_abs(bnerv_ctx* ctx, void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks,
                             unsigned long long k, uint32_t* out) {
    if (int rc = check_table("kth_abs", items, n_items, blocks, n_blocks)) return rc;
    BNERV_REQUIRE(out && aligned(out, 8), "kth_abs: out must be 4 dwords, 8-byte aligned");
    BNERV_REQUIRE(k >= 1 && k <= 0xffffffffull, "kth_abs: k=%llu (1 .. the element count, below 2^32)", k);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned* ws = static_cast<unsigned*>(bnerv_ctx_scratch(ctx, WS_WORDS * sizeof(unsigned), st));
    BNERV_REQUIRE(ws != nullptr, "kth_abs: no scratch for the select state (%zu bytes; context %s)", WS_WORDS * sizeof(unsigned),
                  ctx ? "cannot grow inside a stream capture" : "missing");
    if (hipMemsetAsync(ws, 0, WS_WORDS * sizeof(unsigned), st) != hipSuccess) return bnerv_set_error(BNERV_E_LAUNCH, "kth_abs: memset failed");
    const unsigned* b = reinterpret_cast<const unsigned*>(blocks);
    for (int pass = 0; pass < PASSES; ++pass) {
        if (pass == 0) hipLaunchKernelGGL(kth_hist_kernel<true>, dim3((unsigned)n_blocks), dim3(THREADS), 0, st, items, (unsigned)n_items, b, ws, pass);
        else hipLaunchKernelGGL(kth_hist_kernel<false>, dim3((unsigned)n_blocks), dim3(THREADS), 0, st, items, (unsigned)n_items, b, ws, pass);
        hipLaunchKernelGGL(kth_pick_kernel, dim3(1), dim3(BINS), 0, st, ws, pass, k, reinterpret_cast<unsigned*>(out));
    }
    BNERV_LAUNCH_CHECK("kth_abs");
    return BNERV_OK;
}

extern "C" int bnerv_prune_masks(void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks, const uint32_t* tau_dev) {
    if (int rc = check_table("prune_masks", items, n_items, blocks, n_blocks)) return rc;
    BNERV_REQUIRE(tau_dev && aligned(tau_dev, 4), "prune_masks: tau_dev must be a 4-byte aligned device dword");
    hipLaunchKernelGGL(mask_items_kernel<true>, dim3((unsigned)n_blocks), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), items, (unsigned)n_items,
                       reinterpret_cast<const unsigned*>(blocks), reinterpret_cast<const unsigned*>(tau_dev));
    BNERV_LAUNCH_CHECK("prune_masks");
    return BNERV_OK;
}

extern "C" int bnerv_mask_mul(void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks) {
    if (int rc = check_table("mask_mul", items, n_items, blocks, n_blocks)) return rc;
    hipLaunchKernelGGL(mask_items_kernel<false>, dim3((unsigned)n_blocks), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), items, (unsigned)n_items,
                       reinterpret_cast<const unsigned*>(blocks), static_cast<const unsigned*>(nullptr));
    BNERV_LAUNCH_CHECK("mask_mul");
    return BNERV_OK;
}

extern "C" int bnerv_grad_mask_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const unsigned char* const* masks_dev) {
    BNERV_REQUIRE(table_dev && masks_dev, "grad_mask_table: null args");
    BNERV_REQUIRE(n_tensors > 0 && total_blocks > 0, "grad_mask_table: n_tensors=%d total_blocks=%d", n_tensors, total_blocks);
    BNERV_REQUIRE(aligned(masks_dev, 8), "grad_mask_table: masks_dev must be 8-byte aligned (pointers)");
    hipLaunchKernelGGL(grad_mask_table_kernel, dim3(total_blocks), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), table_dev, n_tensors, masks_dev);
    BNERV_LAUNCH_CHECK("grad_mask_table");
    return BNERV_OK;
}
