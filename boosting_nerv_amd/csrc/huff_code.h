// huff_code.h -- the canonical Huffman code of a qstream file from its 257 code lengths (host code; shared by the host coder huff.cpp and
// the launcher of the decode kernel huff.hip; include/bnerv.h states the conventions).  HuffCodeT<266> is the code of a zstream file
// (huffz.cpp, huffz.hip): the same construction over more leaves, the EOF leaf still the last one.
//
// Leaves are ordered by (length, leaf index); the first code of the shortest length is 0 and every next leaf takes the previous code + 1,
// shifted left by the growth in length.  A decoder looks at the next 32 bits of the string as one left-aligned number w: the leaf has the
// smallest length l with w < limit[l], and is sorted[offset[l] + (w >> (32 - l)) - first[l]].
#pragma once
#include <stdint.h>
#include "../../include/bnerv.h"

template <int LEAVES>
struct HuffCodeT {
    uint32_t code[LEAVES];                  // right-aligned code of every used leaf
    uint64_t limit[33];                     // left-aligned end (exclusive) of the codes of length <= l; limit[longest] == 2^32
    uint32_t first[33];                     // right-aligned first code of length l
    uint16_t offset[33];                    // position in `sorted` of the first leaf of length l
    uint16_t sorted[LEAVES];                // used leaves by (length, index); the rest 0
    int n_used, max_len;
};
using HuffCode = HuffCodeT<BNERV_HUFF_LEAVES>;

// nullptr when the lengths describe a complete prefix code (every length <= 32, the EOF leaf used, Kraft equality); the reason otherwise
template <int LEAVES>
static inline const char* huff_code_build(const unsigned char* len, HuffCodeT<LEAVES>& c) {
    uint64_t kraft = 0;
    c.n_used = 0;
    c.max_len = 0;
    for (int i = 0; i < LEAVES; ++i) {
        c.code[i] = 0;
        c.sorted[i] = 0;
        if (len[i] > 32) return "a code length exceeds 32";
        if (len[i]) { kraft += (uint64_t)1 << (32 - len[i]); c.max_len = len[i] > c.max_len ? len[i] : c.max_len; }
    }
    if (len[LEAVES - 1] == 0) return "the EOF leaf has no code";
    if (kraft != ((uint64_t)1 << 32)) return "the code lengths break Kraft equality";
    uint64_t code = 0;
    c.limit[0] = 0; c.first[0] = 0; c.offset[0] = 0;
    for (int l = 1; l <= 32; ++l) {
        code <<= 1;
        c.first[l] = (uint32_t)code;
        c.offset[l] = (uint16_t)c.n_used;
        for (int i = 0; i < LEAVES; ++i)
            if (len[i] == l) { c.code[i] = (uint32_t)code++; c.sorted[c.n_used++] = (uint16_t)i; }
        c.limit[l] = code << (32 - l);
    }
    return nullptr;
}
