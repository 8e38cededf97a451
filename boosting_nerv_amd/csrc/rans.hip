// rans.hip -- the decode kernel of the chunked CEM file (boosting_nerv_amd/rstream.py, codec.Decoder): the range-ANS
// words as they lie in the file -> the model's fp32 parameter tensors and the [N, C, h, w] embedding tensor, in ONE launch.
//
// A block is one wave and serves up to 64 consecutive runs of ONE record (the block table names the record and the first run), so it
// holds one cumulative table in LDS: at most 4097 dwords.  It copies that table and the words of its runs -- they lie back to back --
// to LDS in one coalesced sweep each; then lane k decodes run k sequentially, integer arithmetic only: a 64-bit state that starts as the
// run's last two words,  q = state & (2^24 - 1),  the symbol that owns slot q,  state = (state >> 24) * prob + (q - left),  and a refill
// of one word while the state is below 2^32 and bulk words remain -- the rule of the host decoder (csrc/ans.cpp decode_run), word for word.
// The symbol comes from a first-level table on the top 8 bits of q, built by every block from its cumulative table: the symbol that owns the
// bucket's first slot and the width of the bit-descent search from there to the one that owns its last -- no step at all where one symbol
// owns the bucket, ceil(log2(alphabet)) dependent LDS reads without the table.  (Measured, DESIGN section 27: 0.69 -> 0.43 us per symbol.)
// Every lane decodes exactly the symbol count the descriptors give it and refills only from [its first word, its state words), so damaged
// bits can neither make a lane spin nor move a read outside the run; the run's span itself is clamped to the block's, the block's to the
// uploaded words.  A run that does not end with all its bulk words consumed and state 0 sets bit 0 of the error word.
// Symbols are staged in LDS two to a dword, CH = 64 per lane and round with a lane stride of 33 dwords: LDS stores bank on
// (address / 4) mod 32 per 32-lane half, so 32 dwords apart every lane of a half would hit one bank; 33 apart they hit 32 different ones.
// After each round the wave walks its runs and writes  out[i] = float(lo + index) * scale (+ beta)  with consecutive lanes on consecutive
// elements; longer runs take more rounds, LDS use does not grow with the run length: 58 KB per block, two decode waves per CU.
#include "common.h"

namespace {

constexpr int WAVE = 64, CH = 64, STRIDE = CH / 2 + 1, SPAN_WORDS = 8192, MAX_A = BNERV_RANS_MAX_ALPHABET, PREC = 24;
constexpr int LUT_BITS = 8;
constexpr unsigned MASK = (1u << PREC) - 1u;

// the product and the sum as two IEEE fp32 operations (see codec.hip on the pragma): Scale_T's `quant * scale`, ScaleBeta_T's `+ beta`
__device__ __forceinline__ float dequant1(int q, float s, float b, bool has_beta) {
#pragma clang fp contract(off)
    const float v = (float)q * s;
    return has_beta ? v + b : v;
}

__global__ __launch_bounds__(WAVE) void rans_dequant_kernel(const unsigned* __restrict__ words, const unsigned n_words, const unsigned* __restrict__ run_start,
                                                            const unsigned n_runs, const bnerv_rans_block* __restrict__ blocks,
                                                            const bnerv_rans_item* __restrict__ items, const unsigned n_items,
                                                            const unsigned* __restrict__ tables, const unsigned n_table_words, const unsigned run,
                                                            int* __restrict__ err) {
    __shared__ unsigned cdf[MAX_A + 1];
    __shared__ unsigned span[SPAN_WORDS];
    __shared__ unsigned stage[WAVE * STRIDE];
    __shared__ unsigned lut[1 << LUT_BITS];
    const unsigned lane = threadIdx.x;
    // ---- the block's descriptors, all uniform; anything that points outside the uploaded arrays ends the block before a dependent load
    const bnerv_rans_block b = blocks[blockIdx.x];
    bool ok = b.item < n_items && b.run < n_runs;
    bnerv_rans_item it = {};
    if (ok) it = items[b.item];
    const unsigned A = it.alphabet;
    const unsigned item_runs = ok && it.n ? (it.n - 1u) / run + 1u : 0u;
    ok = ok && it.out != nullptr && A >= 2u && A <= (unsigned)MAX_A && it.table <= n_table_words && A + 1u <= n_table_words - it.table && b.first < item_runs;
    const unsigned live = ok ? (item_runs - b.first < (unsigned)WAVE ? item_runs - b.first : (unsigned)WAVE) : 0u;
    ok = ok && live <= n_runs - b.run;
    unsigned w0 = 0, w1 = 0;
    if (ok) {
        w0 = run_start[b.run];
        w1 = run_start[b.run + live];
        ok = w0 <= w1 && w1 <= n_words;
    }
    if (!ok) {
        if (lane == 0) atomicOr(err, 2);
        return;
    }
    for (unsigned i = lane; i <= A; i += WAVE) cdf[i] = tables[it.table + i];
    // the words of the block's runs go to LDS in one coalesced sweep, so a refill is an LDS read.  A part that does not fit (above 4 bits per
    // symbol at run 1024, 16 at run 256) is read from memory instead; on C1 at run 1024 that form took the same time.
    const unsigned nw = w1 - w0;
    const bool staged = nw <= (unsigned)SPAN_WORDS;
    if (staged)
        for (unsigned i = lane; i < nw; i += WAVE) span[i] = words[w0 + i];
    __syncthreads();
    auto fetch = [&](unsigned i) -> unsigned { return staged ? span[i - w0] : words[i]; };      // callers keep w0 <= i < w1
    // the largest sym in [from, from + 2 * bit) with cdf[sym] <= q, by bit descent.  cdf[A] = 2^24 > q, so a candidate at or past A is never taken
    auto search = [&](unsigned from, unsigned bit, unsigned q) -> unsigned {
        unsigned sym = from;
        for (; bit; bit >>= 1) {
            const unsigned c = sym + bit;
            sym = cdf[c < A ? c : A] <= q ? c : sym;
        }
        return sym;
    };
    const unsigned top = 1u << (31 - __clz((int)(A - 1u)));              // the highest power of two <= A - 1: the first step of a search of the whole table
    // first level: entry e answers every q whose top LUT_BITS bits are e -- the symbol that owns slot e << 16 (low half) and the first step
    // of the search from there to the symbol that owns the bucket's last slot (high half; 0: one symbol owns the whole bucket)
    for (unsigned e = lane; e < (1u << LUT_BITS); e += WAVE) {
        const unsigned a = search(0, top, e << (PREC - LUT_BITS)), z = search(0, top, ((e + 1u) << (PREC - LUT_BITS)) - 1u);
        lut[e] = a | ((z > a ? 1u << (31 - __clz((int)(z - a))) : 0u) << 16);
    }
    __syncthreads();

    // ---- lane k: run b.run + k, words [s, e) inside [w0, w1), the last two of them the state
    const bool active = lane < live;
    const unsigned first_elem = (b.first + lane) * run;                   // (< it.n < 2^31 for an active lane)
    const unsigned cnt = active ? (it.n - first_elem < run ? it.n - first_elem : run) : 0u;
    unsigned next = w0, bulk_end = w0, bad = 0;
    unsigned long long state = 0;
    if (active) {
        unsigned s = run_start[b.run + lane], e = run_start[b.run + lane + 1];
        s = s < w0 ? w0 : (s > w1 ? w1 : s);
        e = e < s ? s : (e > w1 ? w1 : e);
        if (e - s < 2u) {
            bad = 1;                                                      // no state words: decodes zeros from an empty state, refills nothing
            next = bulk_end = s;
        } else {
            next = s;
            bulk_end = e - 2u;
            state = (unsigned long long)fetch(e - 2u) | ((unsigned long long)fetch(e - 1u) << 32);
        }
    }
    const unsigned block_cnt = it.n - b.first * run < run ? it.n - b.first * run : run;      // lane 0's count: no lane has more
    const unsigned rounds = (block_cnt + CH - 1) / CH;
    const bool has_beta = it.has_beta != 0;
    for (unsigned r = 0; r < rounds; ++r) {
        unsigned pack = 0;
        for (unsigned k = 0; k < (unsigned)CH; ++k) {
            unsigned sym = 0;
            if (r * CH + k < cnt) {
                const unsigned q = (unsigned)state & MASK;
                const unsigned ent = lut[q >> (PREC - LUT_BITS)];
                sym = search(ent & 0xffffu, ent >> 16, q);
                const unsigned left = cdf[sym], prob = cdf[sym + 1] - left;
                state = (state >> PREC) * prob + (q - left);
                if ((state >> 32) == 0 && next < bulk_end) state = (state << 32) | fetch(next++);
            }
            pack |= sym << (16 * (k & 1u));
            if (k & 1u) { stage[lane * STRIDE + (k >> 1)] = pack; pack = 0; }
        }
        __syncthreads();
        // store: run rr of the block, element r * CH + lane of it
        const unsigned e = r * CH + lane;
        for (unsigned rr = 0; rr < live; ++rr) {
            const unsigned f = (b.first + rr) * run, c = it.n - f < run ? it.n - f : run;
            if (e < c) {
                const unsigned sym = (stage[rr * STRIDE + (lane >> 1)] >> (16 * (lane & 1u))) & 0xffffu;
                it.out[(size_t)f + e] = dequant1(it.lo + (int)sym, it.scale, it.beta, has_beta);
            }
        }
        __syncthreads();
    }
    if (active && (bad || next != bulk_end || state != 0)) atomicOr(err, 1);
}

}  // namespace

extern "C" int bnerv_rans_dequant(void* stream, const uint32_t* words, size_t n_words, const uint32_t* run_start, size_t n_runs,
                                  const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_rans_item* items, int n_items,
                                  const uint32_t* tables, size_t n_table_words, int run, int* err) {
    BNERV_REQUIRE(words && run_start && blocks && items && tables && err, "rans_dequant: null args");
    BNERV_REQUIRE(run >= BNERV_RANS_MIN_RUN && run <= BNERV_RANS_MAX_RUN && run % WAVE == 0, "rans_dequant: run = %d (a multiple of %d in %d..%d)", run, WAVE,
                  BNERV_RANS_MIN_RUN, BNERV_RANS_MAX_RUN);
    BNERV_REQUIRE(n_words >= 2 && n_words <= 0xffffffffu && n_runs > 0 && n_runs < 0x7fffffffu && n_blocks > 0 && n_blocks <= 0x7fffffffu && n_items > 0
                  && n_table_words >= 3 && n_table_words <= 0xffffffffu, "rans_dequant: n_words=%zu (two of them padding) n_runs=%zu n_blocks=%zu n_items=%d n_table_words=%zu",
                  n_words, n_runs, n_blocks, n_items, n_table_words);
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(run_start) | reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(err)) & 3) == 0,
                  "rans_dequant: words / run_start / tables / err are not 4-byte aligned");
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(blocks) & 15) == 0 && (reinterpret_cast<uintptr_t>(items) & 7) == 0, "rans_dequant: the descriptor tables are not aligned (blocks 16, items 8 bytes)");
    hipLaunchKernelGGL(rans_dequant_kernel, dim3((unsigned)n_blocks), dim3(WAVE), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const unsigned*>(words),
                       (unsigned)n_words, reinterpret_cast<const unsigned*>(run_start), (unsigned)n_runs, blocks, items, (unsigned)n_items,
                       reinterpret_cast<const unsigned*>(tables), (unsigned)n_table_words, (unsigned)run, err);
    BNERV_LAUNCH_CHECK("rans_dequant");
    return BNERV_OK;
}
