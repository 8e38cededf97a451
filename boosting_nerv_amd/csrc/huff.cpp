// huff.cpp -- host Huffman coder of the post-hoc quantised model (boosting_nerv_amd/qstream.py): the encoder of the file
// and the oracle the decode kernel (huff.hip) is tested against.  The code comes from 257 code lengths (huff_code.h); symbols are cut into
// runs of R that never span two items, the bit string is continuous, and every run's bit length is recorded so that a decoder can start
// anywhere -- the kernel gives one lane to every run.
#include "common.h"
#include "huff_code.h"
#include <stdint.h>
#include <vector>

namespace {

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

}  // namespace

extern "C" long bnerv_huff_encode(const unsigned char* symbols, const unsigned* counts, int n_items, const unsigned char* lengths, int R,
                                  uint32_t* words_out, size_t cap_words, unsigned short* run_bits_out, size_t cap_runs) {
    HuffCode c;
    if (!symbols || !counts || !lengths || !run_bits_out || n_items <= 0) { bnerv_set_error(BNERV_E_ARG, "huff_encode: null or empty argument"); return -1; }
    if (R < 1 || R > 2047) { bnerv_set_error(BNERV_E_ARG, "huff_encode: R = %d (a run's bit length must fit 16 bits: 1 <= R <= 2047)", R); return -1; }
    if (const char* why = huff_code_build(lengths, c)) { bnerv_set_error(BNERV_E_ARG, "huff_encode: %s", why); return -1; }
    for (int k = 0; k < n_items; ++k)
        if (counts[k] == 0) { bnerv_set_error(BNERV_E_ARG, "huff_encode: item %d is empty", k); return -1; }
    if (count_runs(counts, n_items, R) > cap_runs) { bnerv_set_error(BNERV_E_ARG, "huff_encode: %zu runs, room for %zu", count_runs(counts, n_items, R), cap_runs); return -1; }
    // pass 1: the bit lengths (and the check that every symbol has a code)
    uint64_t total = 0;
    size_t at = 0, run = 0;
    for (int k = 0; k < n_items; ++k)
        for (unsigned i0 = 0; i0 < counts[k]; i0 += (unsigned)R) {
            const unsigned i1 = counts[k] - i0 < (unsigned)R ? counts[k] : i0 + (unsigned)R;
            unsigned bits = 0;
            for (unsigned i = i0; i < i1; ++i) {
                const unsigned l = lengths[symbols[at + i]];
                if (l == 0) { bnerv_set_error(BNERV_E_ARG, "huff_encode: symbol %d of item %d has no code", (int)symbols[at + i], k); return -1; }
                bits += l;
            }
            run_bits_out[run++] = (unsigned short)bits;
            total += bits;
            if (i1 == counts[k]) { at += counts[k]; break; }
        }
    const size_t n_words = (size_t)((total + 31) / 32);
    if (!words_out || cap_words < n_words) return (long)n_words;
    // pass 2: the bits, most significant first
    uint64_t acc = 0;           // the low `fill` bits are pending
    unsigned fill = 0;
    size_t w = 0, n_sym = at;
    for (size_t i = 0; i < n_sym; ++i) {
        const unsigned l = lengths[symbols[i]];
        acc = (acc << l) | c.code[symbols[i]];
        fill += l;
        if (fill >= 32) { words_out[w++] = (uint32_t)(acc >> (fill - 32)); fill -= 32; }
    }
    if (fill) words_out[w++] = (uint32_t)(acc << (32 - fill));
    return (long)n_words;
}

extern "C" int bnerv_huff_decode(const uint32_t* words, size_t n_words, const unsigned short* run_bits, size_t n_runs, const unsigned* counts, int n_items,
                                 const unsigned char* lengths, int R, unsigned char* symbols_out) {
    HuffCode c;
    BNERV_REQUIRE((words || !n_words) && run_bits && counts && lengths && symbols_out && n_items > 0, "huff_decode: null or empty argument");
    BNERV_REQUIRE(R >= 1 && R <= 2047, "huff_decode: R = %d", R);
    if (const char* why = huff_code_build(lengths, c)) return bnerv_set_error(BNERV_E_ARG, "huff_decode: %s", why);
    for (int k = 0; k < n_items; ++k) BNERV_REQUIRE(counts[k] > 0, "huff_decode: item %d is empty", k);
    BNERV_REQUIRE(count_runs(counts, n_items, R) == n_runs, "huff_decode: the items make %zu runs, %zu lengths given", count_runs(counts, n_items, R), n_runs);
    uint64_t total = 0;
    for (size_t r = 0; r < n_runs; ++r) total += run_bits[r];
    BNERV_REQUIRE((total + 31) / 32 == n_words, "huff_decode: the run lengths add up to %llu bits, the payload has %zu words", (unsigned long long)total, n_words);
    uint64_t pos = 0;
    size_t at = 0, run = 0;
    for (int k = 0; k < n_items; ++k)
        for (unsigned i0 = 0; i0 < counts[k]; i0 += (unsigned)R, ++run) {
            const unsigned i1 = counts[k] - i0 < (unsigned)R ? counts[k] : i0 + (unsigned)R;
            const uint64_t end = pos + run_bits[run];
            for (unsigned i = i0; i < i1; ++i) {
                const uint32_t w = window(words, n_words, pos);
                int l = 1;
                while (l <= 32 && !(w < c.limit[l])) ++l;
                BNERV_REQUIRE(l <= 32, "huff_decode: run %zu: a bit pattern has no code", run);
                const unsigned leaf = c.sorted[c.offset[l] + ((w >> (32 - l)) - c.first[l])];
                pos += (unsigned)l;
                BNERV_REQUIRE(leaf < 256 && pos <= end, "huff_decode: run %zu does not end on its recorded bit", run);
                symbols_out[at + i] = (unsigned char)leaf;
            }
            BNERV_REQUIRE(pos == end, "huff_decode: run %zu does not end on its recorded bit", run);
            if (i1 == counts[k]) { at += counts[k]; ++run; break; }
        }
    return BNERV_OK;
}
