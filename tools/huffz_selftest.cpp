// huffz_selftest.cpp -- the host coder of the sparse post-hoc file (boosting_nerv_amd/csrc/huffz.cpp) under the host sanitizers: round trips
// and damaged input on exactly sized heap buffers, so that a read or write one element past any of them is reported.  CPU only; build and run:
//
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I boosting_nerv_amd/csrc \
//         tools/huffz_selftest.cpp boosting_nerv_amd/csrc/huffz.cpp -o /tmp/huffz_selftest && /tmp/huffz_selftest
//
// Exit status 0 and "huffz_selftest: N checks passed" when every case behaves; a sanitizer report or a failed check otherwise.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <queue>
#include <random>
#include <vector>
#include "../include/bnerv.h"

static char g_error[512];
int bnerv_set_error(int code, const char* fmt, ...) {      // the library's error sink, restated: huffz.cpp calls it on every refusal
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

static int g_checks = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) { fprintf(stderr, "huffz_selftest: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error); exit(1); } \
    } while (0)

namespace {

constexpr int LEAVES = BNERV_HUFFZ_LEAVES, ZERO = BNERV_HUFFZ_ZERO;

// Huffman code lengths over the used leaves plus EOF (count 1)
std::vector<unsigned char> lengths_of(const std::vector<uint64_t>& hist) {
    struct Node { uint64_t w; int id, l, r; };
    std::vector<Node> nodes;
    auto cmp = [&](int a, int b) { return nodes[a].w != nodes[b].w ? nodes[a].w > nodes[b].w : nodes[a].id > nodes[b].id; };
    std::priority_queue<int, std::vector<int>, decltype(cmp)> heap(cmp);
    for (int i = 0; i < LEAVES; ++i) {
        const uint64_t w = i == LEAVES - 1 ? 1 : hist[i];
        if (w) { nodes.push_back({w, i, -1, -1}); heap.push((int)nodes.size() - 1); }
    }
    std::vector<unsigned char> len(LEAVES, 0);
    if (nodes.size() == 1) { len[nodes[0].id] = 1; return len; }
    nodes.reserve(2 * nodes.size());
    while (heap.size() > 1) {
        const int a = heap.top(); heap.pop();
        const int b = heap.top(); heap.pop();
        nodes.push_back({nodes[a].w + nodes[b].w, LEAVES + (int)nodes.size(), a, b});
        heap.push((int)nodes.size() - 1);
    }
    std::function<void(int, int)> walk = [&](int n, int d) {
        if (nodes[n].l < 0) { len[nodes[n].id] = (unsigned char)d; return; }
        walk(nodes[n].l, d + 1);
        walk(nodes[n].r, d + 1);
    };
    walk(heap.top(), 0);
    return len;
}

std::vector<uint64_t> histogram(const std::vector<unsigned char>& sym, const std::vector<unsigned char>& keep, const std::vector<unsigned>& counts, int parse, int R) {
    std::vector<uint64_t> h(LEAVES, 0);
    size_t at = 0;
    for (unsigned c : counts) {
        for (unsigned i0 = 0; i0 < c; i0 += (unsigned)R) {
            const unsigned n = std::min<unsigned>((unsigned)R, c - i0);
            unsigned z = 0;
            auto flush = [&]() {
                if (parse == BNERV_HUFFZ_SINGLE) h[ZERO] += z;
                else for (int k = 0; k < BNERV_HUFFZ_ZERO_LEAVES; ++k) h[ZERO + k] += (z >> k) & 1u;
                z = 0;
            };
            for (unsigned i = 0; i < n; ++i) {
                if (keep[at + i0 + i]) { flush(); ++h[sym[at + i0 + i]]; } else ++z;
            }
            flush();
        }
        at += c;
    }
    return h;
}

struct Coded { std::vector<uint32_t> words; std::vector<unsigned short> run_bits; std::vector<unsigned char> lengths; };

Coded encode(const std::vector<unsigned char>& sym, const std::vector<unsigned char>& keep, const std::vector<unsigned>& counts, int parse, int R) {
    Coded c;
    c.lengths = lengths_of(histogram(sym, keep, counts, parse, R));
    size_t runs = 0;
    for (unsigned n : counts) runs += (n + (unsigned)R - 1) / (unsigned)R;
    c.run_bits.assign(runs, 0);
    const long need = bnerv_huffz_encode(sym.data(), keep.data(), counts.data(), (int)counts.size(), c.lengths.data(), parse, R, nullptr, 0, c.run_bits.data(), runs);
    CHECK(need >= 0);
    uint64_t total = 0;
    for (unsigned short b : c.run_bits) total += b;
    CHECK((uint64_t)need == (total + 31) / 32);
    c.words.assign((size_t)need, 0xdeadbeefu);                           // exactly sized: a write past it is a heap overflow
    CHECK(bnerv_huffz_encode(sym.data(), keep.data(), counts.data(), (int)counts.size(), c.lengths.data(), parse, R, c.words.data(), c.words.size(), c.run_bits.data(), runs) == need);
    if (need > 0)                                                        // a buffer one word short: the size again, nothing written
        CHECK(bnerv_huffz_encode(sym.data(), keep.data(), counts.data(), (int)counts.size(), c.lengths.data(), parse, R, c.words.data(), c.words.size() - 1, c.run_bits.data(), runs) == need);
    CHECK(bnerv_huffz_encode(sym.data(), keep.data(), counts.data(), (int)counts.size(), c.lengths.data(), parse, R, nullptr, 0, c.run_bits.data(), runs - 1) == -1 || runs == 0);
    return c;
}

int decode(const Coded& c, const std::vector<unsigned>& counts, int R, std::vector<unsigned char>& sym, std::vector<unsigned char>& keep) {
    size_t n = 0;
    for (unsigned v : counts) n += v;
    sym.assign(n, 0xaa);
    keep.assign(n, 0xaa);
    return bnerv_huffz_decode(c.words.data(), c.words.size(), c.run_bits.data(), c.run_bits.size(), counts.data(), (int)counts.size(), c.lengths.data(), R, sym.data(), keep.data());
}

void round_trip(const std::vector<unsigned char>& keep_in, const std::vector<unsigned>& counts, std::mt19937& rng, int R = BNERV_HUFF_RUN) {
    std::vector<unsigned char> sym(keep_in.size()), keep(keep_in);
    for (size_t i = 0; i < sym.size(); ++i) sym[i] = keep[i] ? (unsigned char)(100 + (int)(rng() % 40)) : (unsigned char)(rng() & 255);      // bytes under a zero are ignored
    for (int parse : {BNERV_HUFFZ_SINGLE, BNERV_HUFFZ_RUNS}) {
        const Coded c = encode(sym, keep, counts, parse, R);
        std::vector<unsigned char> s2, k2;
        CHECK(decode(c, counts, R, s2, k2) == BNERV_OK);
        for (size_t i = 0; i < sym.size(); ++i) CHECK(k2[i] == (keep[i] ? 1 : 0) && s2[i] == (keep[i] ? sym[i] : 0));
        // damaged input: every refusal, and never a read or write outside the buffers
        if (c.run_bits.size() >= 2 && c.run_bits[0] && c.run_bits[1]) {
            Coded d = c;
            d.run_bits[0] += 1; d.run_bits[1] -= 1;
            CHECK(decode(d, counts, R, s2, k2) == BNERV_E_ARG);
        }
        if (!c.words.empty()) {
            Coded d = c;
            d.words.pop_back();
            CHECK(decode(d, counts, R, s2, k2) == BNERV_E_ARG && strstr(g_error, "add up"));
            d = c;
            d.run_bits.pop_back();
            CHECK(decode(d, counts, R, s2, k2) == BNERV_E_ARG);
            for (int trial = 0; trial < 8; ++trial) {                    // flipped payload bits: OK or a refusal, the sanitizers watch the rest
                d = c;
                d.words[rng() % d.words.size()] ^= 1u << (rng() % 32);
                const int rc = decode(d, counts, R, s2, k2);
                CHECK(rc == BNERV_OK || rc == BNERV_E_ARG);
            }
            std::vector<unsigned> shorter(counts);                       // an element count below what the bits encode
            if (shorter.back() > 1) {
                shorter.back() -= 1;
                size_t runs = 0;
                for (unsigned v : shorter) runs += (v + (unsigned)R - 1) / (unsigned)R;
                if (runs == c.run_bits.size()) CHECK(decode(c, shorter, R, s2, k2) == BNERV_E_ARG);
            }
        }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    auto random_keep = [&](size_t n, double p) {
        std::vector<unsigned char> k(n);
        for (auto& v : k) v = (rng() / 4294967296.0) < p;
        return k;
    };
    for (double p : {0.0, 0.1, 0.6, 1.0})
        for (unsigned n : {1u, 2u, 255u, 256u, 257u, 511u, 1000u, 70001u}) round_trip(random_keep(n, p), {n}, rng);
    round_trip(random_keep(3 + 300 + 1 + 256, 0.5), {3, 300, 1, 256}, rng);
    round_trip(random_keep(900, 0.3), {900}, rng, 100);
    {   // stretches of 1, 2, 3, 255 and 256 zeros, one over a run's edge, zeros and kept elements alternating
        std::vector<unsigned char> k(5 * 256, 1);
        for (int i : {1, 3, 4, 6, 7, 8}) k[i] = 0;
        std::fill(k.begin() + 250, k.begin() + 263, 0);
        std::fill(k.begin() + 513, k.begin() + 768, 0);
        std::fill(k.begin() + 768, k.begin() + 1024, 0);
        for (int i = 1024; i < 1280; i += 2) k[i] = 0;
        round_trip(k, {5 * 256}, rng);
    }
    {   // codes by hand: leaf 5 is `0`, the leaf of four zeros `10`, EOF `11`
        std::vector<unsigned char> len(LEAVES, 0);
        len[5] = 1; len[ZERO + 2] = 2; len[LEAVES - 1] = 2;
        Coded c;
        c.lengths = len;
        c.run_bits = {3};
        std::vector<unsigned char> s, k;
        c.words = {0xC0000000u};                                         // EOF, then leaf 5
        CHECK(decode(c, {2}, 256, s, k) == BNERV_E_ARG && strstr(g_error, "EOF"));
        c.words = {0x40000000u};                                         // leaf 5, then four zeros
        CHECK(decode(c, {3}, 256, s, k) == BNERV_E_ARG && strstr(g_error, "past its 3 elements"));
        CHECK(decode(c, {5}, 256, s, k) == BNERV_OK && s[0] == 5 && k[0] == 1 && !k[1] && !k[4] && !s[4]);
        CHECK(decode(c, {6}, 256, s, k) == BNERV_E_ARG);                 // the run ends before its sixth element: the next pattern passes the recorded bit
        len[5] = 2;                                                      // Kraft inequality
        c.lengths = len;
        CHECK(decode(c, {5}, 256, s, k) == BNERV_E_ARG && strstr(g_error, "Kraft"));
        const unsigned char sym[2] = {5, 0}, keep[2] = {1, 0};
        const unsigned cnt[1] = {2};
        unsigned short rb[1];
        std::vector<unsigned char> no_zero(LEAVES, 0);
        no_zero[5] = 1; no_zero[LEAVES - 1] = 1;
        CHECK(bnerv_huffz_encode(sym, keep, cnt, 1, no_zero.data(), BNERV_HUFFZ_SINGLE, 256, nullptr, 0, rb, 1) == -1 && strstr(g_error, "has no code"));
        CHECK(bnerv_huffz_encode(sym, keep, cnt, 1, no_zero.data(), 2, 256, nullptr, 0, rb, 1) == -1);
        CHECK(bnerv_huffz_encode(sym, keep, cnt, 1, no_zero.data(), BNERV_HUFFZ_RUNS, 512, nullptr, 0, rb, 1) == -1);
        CHECK(bnerv_huffz_encode(nullptr, keep, cnt, 1, no_zero.data(), BNERV_HUFFZ_RUNS, 256, nullptr, 0, rb, 1) == -1);
        CHECK(bnerv_huffz_decode(nullptr, 1, rb, 1, cnt, 1, no_zero.data(), 256, s.data(), k.data()) == BNERV_E_ARG);
    }
    printf("huffz_selftest: %d checks passed\n", g_checks);
    return 0;
}
