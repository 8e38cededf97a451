// huff.hip -- the decode kernel of the post-hoc quantised model's file (boosting_nerv_amd/qstream.py, codec.Decoder):
// the coded bytes as they lie in the file -> the model's fp32 parameter tensors, in ONE launch.
//
// A block is one wave.  It copies its part of the bit string to LDS, then lane k Huffman-decodes run 64 * block + k sequentially: a 64-bit
// window of the string in registers, refilled one word at a time from a word read one refill ahead; a first-level table of 2^L
// (leaf, length) entries in LDS, built by every block from the canonical tables the launcher passes by value; codes longer than L bits
// take the canonical search, 31 - L compares against limits held in scalar registers.  Every lane decodes exactly the symbol count of
// its run (known from the descriptors, never from the data) and every symbol takes a bounded number of steps, so damaged bits cannot make
// a lane spin; every payload read is clamped to the words that were staged or uploaded, whose last two are zero padding.  A lane whose run
// does not end on the next descriptor's start bit, or that decodes the EOF leaf, sets the error word.
// The symbols of a run are packed four to a dword and staged in LDS with a run stride of 65 dwords: LDS stores bank on (address / 4) mod 32,
// so 64 dwords apart every lane of a 32-lane group would hit one bank; 65 apart they hit 32 different ones.  The wave then walks its 64
// runs, loading the grids of one while it stores the one before, and writes  out[i] = float(min[s]) + float(scale[s]) * float(q[i])  with consecutive lanes on consecutive elements.
//
// The kernel is a template on that last step.  bnerv_huff_decode_u8 (the embedding strings of a pstream file) is the same
// decode body with a store that lets the staged symbols leave as the bytes they are; both entry points go through one launcher.
#include "common.h"
#include "huff_code.h"
#include "huff_rebuild.h"

namespace {

constexpr int RUN = BNERV_HUFF_RUN, LUT_BITS = BNERV_HUFF_LUT_BITS, WAVE = 64, STRIDE = RUN / 4 + 1, SPAN_WORDS = WAVE * RUN / 2;
static_assert(RUN % 4 == 0 && RUN % WAVE == 0, "a run is whole dwords and whole store rounds");

struct Tables {
    unsigned long long limit[33];
    unsigned first[33];
    unsigned short offset[33];
    unsigned short sorted[BNERV_HUFF_LEAVES];
};

// What an instantiation of the kernel does with the decoded symbols: `Item` is the descriptor a run names, `Meta` what the store phase needs
// of every run, left in LDS by the lane that decoded it (a chain of dependent loads per run otherwise); count() is the number of symbols of
// the run that starts at element `first` of its item (0: no such run), note() fills Meta and store() writes the 64 runs of the block from
// the staged symbols (cnt[rr] of them in run rr).

// out[i] = float(min[s]) + float(scale[s]) * float(q[i]): bnerv_huff_dequant
struct FloatStore {
    typedef bnerv_huff_item Item;
    struct Meta {
        float* out[WAVE];
        const void* mn[WAVE];
        const void* sc[WAVE];
        unsigned ri[WAVE], inner[WAVE], first[WAVE];
        int dtype[WAVE];
    };
    static __device__ __forceinline__ unsigned count(const Item& it, const unsigned first) {
        if (first < it.n && it.red != 0 && it.inner != 0) return it.n - first < (unsigned)RUN ? it.n - first : (unsigned)RUN;
        return 0u;
    }
    static __device__ __forceinline__ void note(Meta& m, const unsigned lane, const Item& it, const unsigned first) {
        const unsigned ri = it.red * it.inner;
        m.out[lane] = it.out + first; m.mn[lane] = it.min; m.sc[lane] = it.scale; m.dtype[lane] = it.dtype;
        m.first[lane] = first; m.inner[lane] = it.inner;
        m.ri[lane] = (ri >= it.n && it.inner == 1) ? 0u : ri;              // 0: one (min, scale) pair for the whole tensor
    }
    // One run per step, software-pipelined two deep: the grid loads of the next run are in flight while this one is stored.
    // Every load is unconditional (lanes past the run's end repeat its last element) and the dtype branch is per run, so the eight loads
    // of a run leave together and cost one memory round trip.
    static __device__ __forceinline__ void store(const Meta& m, const unsigned* stage, const unsigned* cnt, const unsigned lane) {
        constexpr int ROUNDS = RUN / WAVE;
        struct Grid { float mn[ROUNDS], sc[ROUNDS]; };
        auto load_run = [&](unsigned rr, Grid& g) {
            const unsigned c = __builtin_amdgcn_readfirstlane(cnt[rr]);
            if (c == 0) return;
            const unsigned ri = __builtin_amdgcn_readfirstlane(m.ri[rr]), inner = __builtin_amdgcn_readfirstlane(m.inner[rr]);
            const unsigned first = __builtin_amdgcn_readfirstlane(m.first[rr]);
            const void* pm = m.mn[rr];
            const void* ps = m.sc[rr];
            unsigned s[ROUNDS];
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const unsigned e = (unsigned)j * WAVE + lane, i = first + (e < c ? e : c - 1);
                s[j] = ri ? (i / ri) * inner + i % inner : 0u;
            }
            if (__builtin_amdgcn_readfirstlane(m.dtype[rr]) == BNERV_HUFF_F16) {
#pragma unroll
                for (int j = 0; j < ROUNDS; ++j) { g.mn[j] = (float)static_cast<const _Float16*>(pm)[s[j]]; g.sc[j] = (float)static_cast<const _Float16*>(ps)[s[j]]; }
            } else {
#pragma unroll
                for (int j = 0; j < ROUNDS; ++j) { g.mn[j] = static_cast<const float*>(pm)[s[j]]; g.sc[j] = static_cast<const float*>(ps)[s[j]]; }
            }
        };
        auto store_run = [&](unsigned rr, const Grid& g) {
            const unsigned c = __builtin_amdgcn_readfirstlane(cnt[rr]);
            if (c == 0) return;
            float* out = m.out[rr];
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const unsigned e = (unsigned)j * WAVE + lane;
                if (e < c) out[e] = rebuild1(g.mn[j], g.sc[j], (stage[rr * STRIDE + (e >> 2)] >> (8 * (e & 3))) & 255u);
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
};

// out[i] = q[i], a byte: bnerv_huff_decode_u8.  A staged dword holds four consecutive symbols in memory order, so lane k of a run owns its
// bytes 4k .. 4k + 3 and writes them as wide as the address of the run's first byte allows: a dword, two halves or four bytes; the
// quad the run ends in goes byte by byte.  Consecutive lanes write consecutive quads: a whole run is one 256-byte sweep.
struct ByteStore {
    typedef bnerv_huff_item_u8 Item;
    struct Meta { unsigned char* out[WAVE]; };
    static_assert(RUN == 4 * WAVE, "a lane owns one staged dword of every run");
    static __device__ __forceinline__ unsigned count(const Item& it, const unsigned first) {
        if (first < it.n) return it.n - first < (unsigned)RUN ? it.n - first : (unsigned)RUN;
        return 0u;
    }
    static __device__ __forceinline__ void note(Meta& m, const unsigned lane, const Item& it, const unsigned first) { m.out[lane] = it.out + first; }
    static __device__ __forceinline__ void store(const Meta& m, const unsigned* stage, const unsigned* cnt, const unsigned lane) {
        for (unsigned rr = 0; rr < (unsigned)WAVE; ++rr) {
            const unsigned c = __builtin_amdgcn_readfirstlane(cnt[rr]);
            if (c == 0) continue;
            unsigned char* p = m.out[rr] + 4u * lane;
            const unsigned e = 4u * lane, v = stage[rr * STRIDE + lane];
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            if (e + 4u <= c) {
                if ((a & 3u) == 0) *reinterpret_cast<unsigned*>(p) = v;
                else if ((a & 1u) == 0) {
                    *reinterpret_cast<unsigned short*>(p) = (unsigned short)(v & 0xffffu);
                    *reinterpret_cast<unsigned short*>(p + 2) = (unsigned short)(v >> 16);
                } else {
                    p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24);
                }
            } else {
                for (unsigned j = 0; j < 4u; ++j)
                    if (e + j < c) p[j] = (unsigned char)(v >> (8u * j));
            }
        }
    }
};

template <class Store>
__global__ __launch_bounds__(WAVE) void huff_decode_kernel(const unsigned* __restrict__ words, const size_t n_words, const bnerv_huff_run* __restrict__ runs,
                                                           const unsigned n_runs, const typename Store::Item* __restrict__ items, const unsigned n_items,
                                                           const Tables t, int* __restrict__ err) {
    __shared__ unsigned stage[WAVE * STRIDE];
    __shared__ unsigned span[SPAN_WORDS];
    __shared__ unsigned s_base[33];                        // offset[l] - first[l] (mod 2^32): leaf = sorted[base[l] + code]
    __shared__ unsigned short s_sorted[BNERV_HUFF_LEAVES], lut[1 << LUT_BITS];
    __shared__ typename Store::Meta meta;
    __shared__ unsigned r_cnt[WAVE];
    const unsigned lane = threadIdx.x;
    for (unsigned i = lane; i < BNERV_HUFF_LEAVES; i += WAVE) s_sorted[i] = t.sorted[i];
    if (lane < 33) s_base[lane] = (unsigned)t.offset[lane] - t.first[lane];
    // the block's part of the bit string -- its runs lie back to back -- goes to LDS in one coalesced sweep: a lane that fetched its words
    // from memory would make the whole wave wait for a load at nearly every symbol.  A part that does not fit (above 16 bits per symbol
    // on average) is read from memory instead.
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
    // first level: entry e answers every window that starts with the LUT_BITS bits e; 0 = the code is longer.  The limits never decrease, so a
    // code's length is 1 + the number of limits at or below the window: compares against kernel arguments (scalar registers), no memory
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
            const typename Store::Item it = items[d.item];
            cnt = Store::count(it, d.first);
            Store::note(meta, lane, it, d.first);
        }
    }
    r_cnt[lane] = cnt;                                   // 0: nothing to decode or store (no such run)
    size_t wi = (size_t)(start >> 5);
    unsigned sh = (unsigned)(start & 31);
    unsigned long long buf = ((unsigned long long)fetch(wi) << 32) | fetch(wi + 1);
    wi += 2;
    unsigned ahead = fetch(wi);                          // the word the next refill shifts in, read one refill early
    unsigned bits = 0, bad = 0, pack = 0;
    for (int k = 0; k < RUN; ++k) {
        if ((unsigned)k < cnt) {
            const unsigned w = (unsigned)((buf << sh) >> 32);
            const unsigned ent = lut[w >> (32 - LUT_BITS)];
            unsigned len = ent >> 9, leaf = ent & 511u;
            if (len == 0) {
                // LUT_BITS + 1 + the number of longer limits at or below the window, as above: 21 compares, no memory, no branch -- one lane
                // with a long code makes its whole wave walk this path
                len = LUT_BITS + 1;
#pragma unroll
                for (int l = LUT_BITS + 1; l < 32; ++l) len += (unsigned long long)w >= t.limit[l] ? 1u : 0u;
                leaf = s_sorted[s_base[len] + (w >> (32 - len))];
            }
            if (leaf > 255u) { bad = 1; leaf = 0; }
            bits += len;
            sh += len;
            if (sh >= 32) {
                buf = (buf << 32) | ahead;
                ++wi;
                ahead = fetch(wi);
                sh -= 32;
            }
            pack |= leaf << (8 * (k & 3));
        }
        if ((k & 3) == 3) { stage[lane * STRIDE + (k >> 2)] = pack; pack = 0; }
    }
    if (active && (bad || start + bits != next)) atomicOr(err, 1);
    __syncthreads();

    Store::store(meta, stage, r_cnt, lane);
}

// the checks, the canonical tables and the launch both entry points share
template <class Store>
int launch(const char* who, void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs, const typename Store::Item* items,
           int n_items, const unsigned char* lengths_host, int R, int* err) {
    BNERV_REQUIRE(words && runs && items && lengths_host && err, "%s: null args", who);
    BNERV_REQUIRE(R == BNERV_HUFF_RUN, "%s: R = %d (the kernel is built for runs of %d)", who, R, BNERV_HUFF_RUN);
    BNERV_REQUIRE(n_words >= 3 && n_runs > 0 && n_runs <= 0x7fffffffu / WAVE && n_items > 0, "%s: n_words=%zu (two of them padding) n_runs=%zu n_items=%d", who,
                  n_words, n_runs, n_items);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(words) & 3) == 0 && (reinterpret_cast<uintptr_t>(err) & 3) == 0, "%s: words / err are not 4-byte aligned", who);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(runs) & 7) == 0 && (reinterpret_cast<uintptr_t>(items) & 7) == 0, "%s: the descriptor tables are not 8-byte aligned", who);
    HuffCode c;
    if (const char* why = huff_code_build(lengths_host, c)) return bnerv_set_error(BNERV_E_ARG, "%s: %s", who, why);
    Tables t;
    for (int l = 0; l <= 32; ++l) { t.limit[l] = c.limit[l]; t.first[l] = c.first[l]; t.offset[l] = c.offset[l]; }
    for (int i = 0; i < BNERV_HUFF_LEAVES; ++i) t.sorted[i] = c.sorted[i];
    hipLaunchKernelGGL(huff_decode_kernel<Store>, dim3((unsigned)((n_runs + WAVE - 1) / WAVE)), dim3(WAVE), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned*>(words), n_words, runs, (unsigned)n_runs, items, (unsigned)n_items, t, err);
    BNERV_LAUNCH_CHECK(who);
    return BNERV_OK;
}

}  // namespace

extern "C" int bnerv_huff_dequant(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                                  const bnerv_huff_item* items, int n_items, const unsigned char* lengths_host, int R, int* err) {
    return launch<FloatStore>("huff_dequant", stream, words, n_words, runs, n_runs, items, n_items, lengths_host, R, err);
}

extern "C" int bnerv_huff_decode_u8(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                                    const bnerv_huff_item_u8* items, int n_items, const unsigned char* lengths_host, int R, int* err) {
    return launch<ByteStore>("huff_decode_u8", stream, words, n_words, runs, n_runs, items, n_items, lengths_host, R, err);
}
