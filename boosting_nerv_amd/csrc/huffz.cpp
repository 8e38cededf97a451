// huffz.cpp -- host Huffman coder of the sparse post-hoc quantised model (boosting_nerv_amd/zstream.py): the encoder of
// the file and the oracle the decode kernel (huffz.hip) is tested against.  huff.cpp's coder with leaves for zeros: the code comes from 266
// code lengths (huff_code.h), the ELEMENTS of an item are cut into runs of R that never span two items, a stretch of zero elements is
// clipped at its run's ends and written as zero-run leaves, and every run's bit length is recorded.
// Plain C++ (no HIP header), so that tools/huffz_selftest.cpp can build it under the host sanitizers.
#include "huff_code.h"
#include <stddef.h>
#include <stdint.h>

int bnerv_set_error(int code, const char* fmt, ...);

#define HUFFZ_REQUIRE(cond, ...)                                   \
    do {                                                           \
        if (!(cond)) return bnerv_set_error(BNERV_E_ARG, __VA_ARGS__); \
    } while (0)

namespace {

using Code = HuffCodeT<BNERV_HUFFZ_LEAVES>;
constexpr unsigned ZERO = BNERV_HUFFZ_ZERO, EOF_LEAF = BNERV_HUFFZ_LEAVES - 1;

// the 32 bits at bit `pos` of the string as one left-aligned number; bits behind the last word read as 0
inline uint32_t window(const uint32_t* words, size_t n_words, uint64_t pos) {
    const size_t wi = (size_t)(pos >> 5);
    const unsigned sh = (unsigned)(pos & 31);
    const uint64_t hi = wi < n_words ? words[wi] : 0u, lo = wi + 1 < n_words ? words[wi + 1] : 0u;
    return (uint32_t)((((hi << 32) | lo) << sh) >> 32);
}

size_t count_runs(const unsigned* counts, int n_items, int R) {
    size_t n = 0;
    for (int k = 0; k < n_items; ++k) n += ((size_t)counts[k] + (size_t)R - 1) / (size_t)R;
    return n;
}

struct Writer {
    uint32_t* words;            // nullptr: count only
    uint64_t acc = 0;           // the low `fill` bits are pending
    unsigned fill = 0;
    size_t w = 0;
    void put(uint32_t code, unsigned l) {
        if (!words) return;
        acc = (acc << l) | code;
        fill += l;
        if (fill >= 32) { words[w++] = (uint32_t)(acc >> (fill - 32)); fill -= 32; }
    }
    void flush() {
        if (words && fill) { words[w++] = (uint32_t)(acc << (32 - fill)); fill = 0; }
    }
};

// the leaves of one run of `n` elements, in order; emit(leaf) returns false to stop
template <class Emit>
bool parse_run(const unsigned char* sym, const unsigned char* keep, unsigned n, int parse, Emit emit) {
    unsigned i = 0;
    while (i < n) {
        if (keep[i]) {
            if (!emit((unsigned)sym[i])) return false;
            ++i;
            continue;
        }
        unsigned z = 0;
        while (i + z < n && !keep[i + z]) ++z;
        i += z;
        if (parse == BNERV_HUFFZ_SINGLE) {
            for (unsigned j = 0; j < z; ++j)
                if (!emit(ZERO)) return false;
        } else {
            for (int k = BNERV_HUFFZ_ZERO_LEAVES - 1; k >= 0; --k)
                if ((z >> k) & 1u)
                    if (!emit(ZERO + (unsigned)k)) return false;
        }
    }
    return true;
}

}  // namespace

extern "C" long bnerv_huffz_encode(const unsigned char* symbols, const unsigned char* keep, const unsigned* counts, int n_items, const unsigned char* lengths,
                                   int parse, int R, uint32_t* words_out, size_t cap_words, unsigned short* run_bits_out, size_t cap_runs) {
    Code c;
    if (!symbols || !keep || !counts || !lengths || !run_bits_out || n_items <= 0) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: null or empty argument"); return -1; }
    if (R < 1 || R > BNERV_HUFF_RUN) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: R = %d (a zero-run leaf covers at most %d elements: 1 <= R <= %d)", R, BNERV_HUFF_RUN, BNERV_HUFF_RUN); return -1; }
    if (parse != BNERV_HUFFZ_SINGLE && parse != BNERV_HUFFZ_RUNS) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: parse = %d", parse); return -1; }
    if (const char* why = huff_code_build(lengths, c)) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: %s", why); return -1; }
    for (int k = 0; k < n_items; ++k)
        if (counts[k] == 0) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: item %d is empty", k); return -1; }
    if (count_runs(counts, n_items, R) > cap_runs) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: %zu runs, room for %zu", count_runs(counts, n_items, R), cap_runs); return -1; }
    // pass 0 counts the bits (and checks that every leaf has a code), pass 1 writes them
    size_t n_words = 0;
    for (int pass = 0; pass < 2; ++pass) {
        Writer out{pass ? words_out : nullptr};
        uint64_t total = 0;
        size_t at = 0, run = 0;
        int missing = -1;
        for (int k = 0; k < n_items; ++k) {
            for (unsigned i0 = 0; i0 < counts[k]; i0 += (unsigned)R) {
                const unsigned n = counts[k] - i0 < (unsigned)R ? counts[k] - i0 : (unsigned)R;
                unsigned bits = 0;
                const bool ok = parse_run(symbols + at + i0, keep + at + i0, n, parse, [&](unsigned leaf) {
                    const unsigned l = lengths[leaf];
                    if (l == 0) { missing = (int)leaf; return false; }
                    bits += l;
                    out.put(c.code[leaf], l);
                    return true;
                });
                if (!ok) { bnerv_set_error(BNERV_E_ARG, "huffz_encode: leaf %d of item %d has no code", missing, k); return -1; }
                if (!pass) run_bits_out[run] = (unsigned short)bits;
                ++run;
                total += bits;
            }
            at += counts[k];
        }
        out.flush();
        n_words = (size_t)((total + 31) / 32);
        if (!words_out || cap_words < n_words) return (long)n_words;
    }
    return (long)n_words;
}

extern "C" int bnerv_huffz_decode(const uint32_t* words, size_t n_words, const unsigned short* run_bits, size_t n_runs, const unsigned* counts, int n_items,
                                  const unsigned char* lengths, int R, unsigned char* symbols_out, unsigned char* keep_out) {
    Code c;
    HUFFZ_REQUIRE((words || !n_words) && run_bits && counts && lengths && symbols_out && keep_out && n_items > 0, "huffz_decode: null or empty argument");
    HUFFZ_REQUIRE(R >= 1 && R <= BNERV_HUFF_RUN, "huffz_decode: R = %d", R);
    if (const char* why = huff_code_build(lengths, c)) return bnerv_set_error(BNERV_E_ARG, "huffz_decode: %s", why);
    for (int k = 0; k < n_items; ++k) HUFFZ_REQUIRE(counts[k] > 0, "huffz_decode: item %d is empty", k);
    HUFFZ_REQUIRE(count_runs(counts, n_items, R) == n_runs, "huffz_decode: the items make %zu runs, %zu lengths given", count_runs(counts, n_items, R), n_runs);
    uint64_t total = 0;
    for (size_t r = 0; r < n_runs; ++r) total += run_bits[r];
    HUFFZ_REQUIRE((total + 31) / 32 == n_words, "huffz_decode: the run lengths add up to %llu bits, the payload has %zu words", (unsigned long long)total, n_words);
    uint64_t pos = 0;
    size_t at = 0, run = 0;
    for (int k = 0; k < n_items; ++k) {
        for (unsigned i0 = 0; i0 < counts[k]; i0 += (unsigned)R, ++run) {
            const unsigned n = counts[k] - i0 < (unsigned)R ? counts[k] - i0 : (unsigned)R;
            const uint64_t end = pos + run_bits[run];
            unsigned char* sym = symbols_out + at + i0;
            unsigned char* kp = keep_out + at + i0;
            unsigned i = 0;
            while (i < n) {
                const uint32_t w = window(words, n_words, pos);
                int l = 1;
                while (l <= 32 && !(w < c.limit[l])) ++l;
                HUFFZ_REQUIRE(l <= 32, "huffz_decode: run %zu: a bit pattern has no code", run);
                const unsigned leaf = c.sorted[c.offset[l] + ((w >> (32 - l)) - c.first[l])];
                pos += (unsigned)l;
                HUFFZ_REQUIRE(leaf != EOF_LEAF, "huffz_decode: run %zu: a bit pattern decodes to EOF", run);
                HUFFZ_REQUIRE(pos <= end, "huffz_decode: run %zu does not end on its recorded bit", run);
                if (leaf < ZERO) {
                    sym[i] = (unsigned char)leaf;
                    kp[i++] = 1;
                } else {
                    const unsigned z = 1u << (leaf - ZERO);
                    HUFFZ_REQUIRE(z <= n - i, "huffz_decode: run %zu: a zero-run leaf of %u elements carries the run past its %u elements", run, z, n);
                    for (unsigned j = 0; j < z; ++j) { sym[i] = 0; kp[i++] = 0; }
                }
            }
            HUFFZ_REQUIRE(pos == end, "huffz_decode: run %zu does not end on its recorded bit", run);
        }
        at += counts[k];
    }
    return BNERV_OK;
}
