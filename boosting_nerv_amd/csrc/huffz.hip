// huffz.hip -- the decode kernel of the sparse post-hoc quantised model's file (boosting_nerv_amd/zstream.py, codec.Decoder; DESIGN
// section 31): the coded bytes as they lie in the file -> the model's fp32 parameter tensors, pruned weights exactly +0.0, in ONE launch.
//
// The skeleton is huff.hip's: a block is one wave; it copies its part of the bit string to LDS (clamped reads of global memory when the part
// outgrows the span), builds the first-level table of 2^L (leaf, length) entries, and lane k decodes run 64 * block + k sequentially from
// a 64-bit window refilled one word at a time, with the canonical search against limits in scalar registers for codes longer than L bits.
// The 16-bit table entry is leaf | length << 9: nine bits of leaf hold the 266 leaves of this alphabet, and a length is at most L = 12.
//
// What is new is the loop: a run is 256 ELEMENTS, not 256 leaves.  A lane runs until it has produced its run's element count (from the
// descriptors, never from the data); a data leaf produces one element, zero-run leaf 256 + k produces 2^k, so every step advances by at least
// one element, the loop takes at most 256 steps, and it ends as soon as no lane of the wave has elements left -- a sparse model takes fewer steps than
// a dense one.  A zero-run leaf that would pass the run's end is clamped to it and, like an EOF leaf or a run that does not end on the next
// descriptor's start bit, sets the error word.
// Next to the packed symbols (run stride 65 dwords, as in huff.hip) every run has a 256-bit keep mask in LDS with a stride of 9 dwords: LDS
// stores bank on (address / 4) mod 32 per 32-lane half, so 8 dwords apart the lanes of a half would share 4 banks and 9 apart they take 32
// different ones.  A lane gathers the symbols of one dword and the keep bits of one mask word in registers and stores each when it moves on;
// the masks are cleared first, so the words a zero run skips stay zero; symbol bytes under a clear keep bit are never looked at.
// The store phase is huff.hip's with one select:  out[i] = keep ? float(min[s]) + float(scale[s]) * float(q[i]) : +0.0f.
#include "common.h"
#include "huff_code.h"
#include "huff_rebuild.h"

namespace {

constexpr int RUN = BNERV_HUFF_RUN, LUT_BITS = BNERV_HUFF_LUT_BITS, WAVE = 64, STRIDE = RUN / 4 + 1, MSTRIDE = RUN / 32 + 1, SPAN_WORDS = WAVE * RUN / 2;
constexpr unsigned ZERO = BNERV_HUFFZ_ZERO, EOF_LEAF = BNERV_HUFFZ_LEAVES - 1;
static_assert(RUN % 32 == 0 && RUN % WAVE == 0, "a run is whole mask words and whole store rounds");
static_assert(BNERV_HUFFZ_LEAVES <= 512 && LUT_BITS < 16, "a table entry is leaf | length << 9 in 16 bits");
static_assert((1 << (BNERV_HUFFZ_ZERO_LEAVES - 1)) <= RUN, "the longest zero-run leaf fits a run");

struct Tables {
    unsigned long long limit[33];
    unsigned first[33];
    unsigned short offset[33];
    unsigned short sorted[BNERV_HUFFZ_LEAVES];
};

__global__ __launch_bounds__(WAVE) void huffz_dequant_kernel(const unsigned* __restrict__ words, const size_t n_words, const bnerv_huff_run* __restrict__ runs,
                                                             const unsigned n_runs, const bnerv_huff_item* __restrict__ items, const unsigned n_items,
                                                             const Tables t, int* __restrict__ err) {
    __shared__ unsigned stage[WAVE * STRIDE];
    __shared__ unsigned mask[WAVE * MSTRIDE];
    __shared__ unsigned span[SPAN_WORDS];
    __shared__ unsigned s_base[33];                        // offset[l] - first[l] (mod 2^32): leaf = sorted[base[l] + code]
    __shared__ unsigned short s_sorted[BNERV_HUFFZ_LEAVES], lut[1 << LUT_BITS];
    // what the store phase needs of every run, left in LDS by the lane that decoded it
    __shared__ float* r_out[WAVE];
    __shared__ const void* r_min[WAVE];
    __shared__ const void* r_scale[WAVE];
    __shared__ unsigned r_cnt[WAVE], r_ri[WAVE], r_inner[WAVE], r_first[WAVE];
    __shared__ int r_dtype[WAVE];
    const unsigned lane = threadIdx.x;
    for (unsigned i = lane; i < BNERV_HUFFZ_LEAVES; i += WAVE) s_sorted[i] = t.sorted[i];
    if (lane < 33) s_base[lane] = (unsigned)t.offset[lane] - t.first[lane];
#pragma unroll
    for (int j = 0; j < RUN / 32; ++j) mask[lane * MSTRIDE + j] = 0u;
    // the block's part of the bit string -- its runs lie back to back -- in one coalesced sweep; a part that does not fit is read from memory
    const size_t last = n_words - 1;                     // a zero word of the padding
    const unsigned r_lo = blockIdx.x * WAVE, r_hi = r_lo + WAVE < n_runs ? r_lo + WAVE : n_runs;
    size_t base = (size_t)(runs[r_lo].start_bit >> 5), end = (size_t)((runs[r_hi].start_bit + 31) >> 5) + 2;
    base = base < last ? base : last;
    end = end < n_words ? end : n_words;
    const size_t nw = end > base ? end - base : 1;
    const bool staged = nw <= (size_t)SPAN_WORDS;
    if (staged)
        for (size_t i = lane; i < nw; i += WAVE) span[i] = words[base + i];
    __syncthreads();
    auto fetch = [&](size_t i) -> unsigned {
        if (staged) {
            const size_t j = i > base ? i - base : 0;
            return span[j < nw ? j : nw - 1];
        }
        return words[i < last ? i : last];
    };
    // first level: entry e answers every window that starts with the LUT_BITS bits e; 0 = the code is longer (huff.hip)
    for (unsigned e = lane; e < (1u << LUT_BITS); e += WAVE) {
        const unsigned w = e << (32 - LUT_BITS);
        unsigned len = 1;
#pragma unroll
        for (int l = 1; l < LUT_BITS; ++l) len += (unsigned long long)w >= t.limit[l] ? 1u : 0u;
        unsigned v = 0;
        if ((unsigned long long)w < t.limit[LUT_BITS]) v = (unsigned)s_sorted[s_base[len] + (w >> (32 - len))] | (len << 9);
        lut[e] = (unsigned short)v;
    }
    __syncthreads();

    const unsigned r = blockIdx.x * WAVE + lane;
    const bool active = r < n_runs;
    unsigned long long start = 0, next = 0;
    unsigned cnt = 0;
    if (active) {
        const bnerv_huff_run d = runs[r];
        start = d.start_bit;
        next = runs[r + 1].start_bit;
        if (d.item < n_items) {
            const bnerv_huff_item it = items[d.item];
            if (d.first < it.n && it.red != 0 && it.inner != 0) cnt = it.n - d.first < (unsigned)RUN ? it.n - d.first : (unsigned)RUN;
            const unsigned ri = it.red * it.inner;
            r_out[lane] = it.out + d.first; r_min[lane] = it.min; r_scale[lane] = it.scale; r_dtype[lane] = it.dtype;
            r_first[lane] = d.first; r_inner[lane] = it.inner;
            r_ri[lane] = (ri >= it.n && it.inner == 1) ? 0u : ri;          // 0: one (min, scale) pair for the whole tensor
        }
    }
    r_cnt[lane] = cnt;                                   // 0: nothing to decode or store (no such run)
    size_t wi = (size_t)(start >> 5);
    unsigned sh = (unsigned)(start & 31);
    unsigned long long buf = ((unsigned long long)fetch(wi) << 32) | fetch(wi + 1);
    wi += 2;
    unsigned ahead = fetch(wi);                          // the word the next refill shifts in, read one refill early
    unsigned bits = 0, bad = 0;
    unsigned pos = 0;                                    // elements produced so far: <= cnt <= RUN at every point
    unsigned pack = 0, pack_at = 0, keep = 0, keep_at = 0;      // the symbol dword and the mask word being gathered, and their indices (< RUN / 4, < RUN / 32)
    // every trip advances every unfinished lane by at least one element: at most RUN trips (the bound is there for the reader and the compiler)
    for (int trip = 0; trip < RUN && __ballot(pos < cnt) != 0ull; ++trip) {
        if (pos < cnt) {
            const unsigned w = (unsigned)((buf << sh) >> 32);
            const unsigned ent = lut[w >> (32 - LUT_BITS)];
            unsigned len = ent >> 9, leaf = ent & 511u;
            if (len == 0) {
                len = LUT_BITS + 1;
#pragma unroll
                for (int l = LUT_BITS + 1; l < 32; ++l) len += (unsigned long long)w >= t.limit[l] ? 1u : 0u;
                const unsigned at = s_base[len] + (w >> (32 - len));
                leaf = s_sorted[at < (unsigned)BNERV_HUFFZ_LEAVES ? at : (unsigned)BNERV_HUFFZ_LEAVES - 1];
            }
            bits += len;
            sh += len;
            if (sh >= 32) {
                buf = (buf << 32) | ahead;
                ++wi;
                ahead = fetch(wi);
                sh -= 32;
            }
            if (leaf < ZERO) {
                const unsigned d = pos >> 2, m = pos >> 5;
                if (d != pack_at) { stage[lane * STRIDE + pack_at] = pack; pack = 0; pack_at = d; }
                if (m != keep_at) { mask[lane * MSTRIDE + keep_at] = keep; keep = 0; keep_at = m; }
                pack |= leaf << (8 * (pos & 3));
                keep |= 1u << (pos & 31);
                pos += 1;
            } else {
                unsigned z = 1u << (leaf - ZERO);        // leaf <= 265: the EOF leaf reads as 512 elements and is clamped like any overrun
                if (leaf == EOF_LEAF || z > cnt - pos) { bad = 1; z = cnt - pos; }
                pos += z;
            }
        }
    }
    stage[lane * STRIDE + pack_at] = pack;
    mask[lane * MSTRIDE + keep_at] = keep;
    if (active && (bad || pos != cnt || start + bits != next)) atomicOr(err, 1);
    __syncthreads();

    // Store phase, one run per step, software-pipelined two deep (huff.hip): the grid loads of the next run are in flight while this one is stored
    constexpr int ROUNDS = RUN / WAVE;
    struct Grid { float mn[ROUNDS], sc[ROUNDS]; };
    auto load_run = [&](unsigned rr, Grid& g) {
        const unsigned c = __builtin_amdgcn_readfirstlane(r_cnt[rr]);
        if (c == 0) return;
        const unsigned ri = __builtin_amdgcn_readfirstlane(r_ri[rr]), inner = __builtin_amdgcn_readfirstlane(r_inner[rr]);
        const unsigned first = __builtin_amdgcn_readfirstlane(r_first[rr]);
        const void* pm = r_min[rr];
        const void* ps = r_scale[rr];
        unsigned s[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const unsigned e = (unsigned)j * WAVE + lane, i = first + (e < c ? e : c - 1);
            s[j] = ri ? (i / ri) * inner + i % inner : 0u;
        }
        if (__builtin_amdgcn_readfirstlane(r_dtype[rr]) == BNERV_HUFF_F16) {
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) { g.mn[j] = (float)static_cast<const _Float16*>(pm)[s[j]]; g.sc[j] = (float)static_cast<const _Float16*>(ps)[s[j]]; }
        } else {
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) { g.mn[j] = static_cast<const float*>(pm)[s[j]]; g.sc[j] = static_cast<const float*>(ps)[s[j]]; }
        }
    };
    auto store_run = [&](unsigned rr, const Grid& g) {
        const unsigned c = __builtin_amdgcn_readfirstlane(r_cnt[rr]);
        if (c == 0) return;
        float* out = r_out[rr];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const unsigned e = (unsigned)j * WAVE + lane;
            if (e < c) {
                const bool k = (mask[rr * MSTRIDE + (e >> 5)] >> (e & 31)) & 1u;
                const float v = rebuild1(g.mn[j], g.sc[j], (stage[rr * STRIDE + (e >> 2)] >> (8 * (e & 3))) & 255u);
                out[e] = k ? v : 0.0f;
            }
        }
    };
    Grid a, b;
    load_run(0, a);
    for (unsigned rr = 0; rr < (unsigned)WAVE; rr += 2) {
        load_run(rr + 1, b);
        store_run(rr, a);
        if (rr + 2 < (unsigned)WAVE) load_run(rr + 2, a);
        store_run(rr + 1, b);
    }
}

}  // namespace

extern "C" int bnerv_huffz_dequant(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                                   const bnerv_huff_item* items, int n_items, const unsigned char* lengths_host, int R, int* err) {
    BNERV_REQUIRE(words && runs && items && lengths_host && err, "huffz_dequant: null args");
    BNERV_REQUIRE(R == BNERV_HUFF_RUN, "huffz_dequant: R = %d (the kernel is built for runs of %d)", R, BNERV_HUFF_RUN);
    BNERV_REQUIRE(n_words >= 3 && n_runs > 0 && n_runs <= 0x7fffffffu / WAVE && n_items > 0, "huffz_dequant: n_words=%zu (two of them padding) n_runs=%zu n_items=%d",
                  n_words, n_runs, n_items);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(words) & 3) == 0 && (reinterpret_cast<uintptr_t>(err) & 3) == 0, "huffz_dequant: words / err are not 4-byte aligned");
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(runs) & 7) == 0 && (reinterpret_cast<uintptr_t>(items) & 7) == 0, "huffz_dequant: the descriptor tables are not 8-byte aligned");
    HuffCodeT<BNERV_HUFFZ_LEAVES> c;
    if (const char* why = huff_code_build(lengths_host, c)) return bnerv_set_error(BNERV_E_ARG, "huffz_dequant: %s", why);
    Tables t;
    for (int l = 0; l <= 32; ++l) { t.limit[l] = c.limit[l]; t.first[l] = c.first[l]; t.offset[l] = c.offset[l]; }
    for (int i = 0; i < BNERV_HUFFZ_LEAVES; ++i) t.sorted[i] = c.sorted[i];
    hipLaunchKernelGGL(huffz_dequant_kernel, dim3((unsigned)((n_runs + WAVE - 1) / WAVE)), dim3(WAVE), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned*>(words), n_words, runs, (unsigned)n_runs, items, (unsigned)n_items, t, err);
    BNERV_LAUNCH_CHECK("huffz_dequant");
    return BNERV_OK;
}
