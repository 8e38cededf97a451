// ans.cpp -- range-ANS entropy coder for the compression report (host code).
//
// Replaces the coder the reference calls for its "real" bit counts: constriction's AnsCoder with a QuantizedGaussian model
// (lib/entropy_model.py:46-62, consumed as `real_bitrate` in train_nerv_compression.py:484-512, 560-577) and with a Categorical
// model (lib/entropy_model.py:65-81).  constriction (a Rust crate with Python bindings) is not part of the reference tree; this
// file restates its published default configuration:
//   * stream code: rANS with a 64-bit state, 32-bit words, 24-bit fixed-point probabilities; symbols are encoded in REVERSE
//     order (stack semantics) so that decoding pops them in message order; the compressed message is the emitted words followed
//     by the non-zero words of the final state;
//   * QuantizedGaussian(min, max, mean, std): the "leaky" quantisation -- every integer in [min, max] owns at least one of the
//     2^24 slots, the remaining 2^24 - n are split by the Gaussian mass of [k - 1/2, k + 1/2), renormalised to the support;
//   * Categorical(p): fixed-point approximation of p with every symbol >= 1 slot.
// Bit-exact equality with constriction's byte stream is NOT claimed (its tie-breaking in the fixed-point rounding is not
// specified by the algorithm); what is tested is decode(encode(x)) == x and  coded bits <= ideal code length * 1.01 + 64.
#include "common.h"
#include <math.h>
#include <stdint.h>
#include <vector>
#include <algorithm>

namespace {

constexpr int PREC = 24;
constexpr uint32_t TOTAL = 1u << PREC;

struct Table {                       // cumulative slot counts: symbol i owns [cdf[i], cdf[i + 1])
    std::vector<uint32_t> cdf;
    int n() const { return (int)cdf.size() - 1; }
};

inline double phi(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

// shift > 0 (the wide runs): entry k is the bucket of the 2^shift integers from lo + (k << shift); the last may be partial
bool gaussian_table(int32_t lo, int32_t hi, double mean, double std, Table& t, int shift = 0) {
    if (hi < lo || shift < 0 || shift > 30 || !(std > 0.0) || !isfinite(mean) || !isfinite(std)) return false;
    const int64_t n = ((int64_t)hi - lo + ((int64_t)1 << shift)) >> shift;
    if (n > (int64_t)TOTAL / 2) return false;
    const double free_slots = (double)(TOTAL - (uint32_t)n);
    const double c0 = phi((lo - 0.5 - mean) / std), c1 = phi((hi + 0.5 - mean) / std);
    const double z = c1 - c0;
    t.cdf.resize((size_t)n + 1);
    t.cdf[0] = 0;
    for (int64_t k = 1; k < n; ++k) {
        double f = z > 0.0 ? (phi((lo + (k << shift) - 0.5 - mean) / std) - c0) / z : (double)k / (double)n;
        f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
        t.cdf[(size_t)k] = (uint32_t)(free_slots * f) + (uint32_t)k;             // leak: one slot per symbol below k
    }
    t.cdf[(size_t)n] = TOTAL;
    for (int64_t k = 1; k <= n; ++k)                                               // monotone by construction; keep it strict
        if (t.cdf[(size_t)k] <= t.cdf[(size_t)k - 1]) return false;
    return true;
}

bool categorical_table(const double* p, int K, Table& t) {
    if (K < 1 || K > (int)(TOTAL / 2)) return false;
    double sum = 0.0;
    for (int i = 0; i < K; ++i) { if (!(p[i] >= 0.0) || !isfinite(p[i])) return false; sum += p[i]; }
    if (!(sum > 0.0)) return false;
    std::vector<uint32_t> f((size_t)K);
    const double free_slots = (double)(TOTAL - (uint32_t)K);
    uint64_t used = 0;
    for (int i = 0; i < K; ++i) { f[(size_t)i] = 1u + (uint32_t)(free_slots * (p[i] / sum)); used += f[(size_t)i]; }
    // hand the slots lost to truncation to the most probable symbols (largest first, index order on ties)
    std::vector<int> order((size_t)K);
    for (int i = 0; i < K; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p[a] > p[b]; });
    for (size_t j = 0; used < TOTAL; j = (j + 1) % (size_t)K) { ++f[(size_t)order[j]]; ++used; }
    t.cdf.resize((size_t)K + 1);
    t.cdf[0] = 0;
    for (int i = 0; i < K; ++i) t.cdf[(size_t)i + 1] = t.cdf[(size_t)i] + f[(size_t)i];
    return t.cdf[(size_t)K] == TOTAL;
}

// symbols are table indices 0 .. n-1
// two_state_words: the final state always takes two words (low, high), zero ones included -- the runs of the chunked layout
// shift > 0: sym[i] = (table index << shift) | low; per symbol the low bits go in first, as `shift` raw bits under the implicit uniform
// table (left = low << (24 - shift), prob = 1 << (24 - shift)), then the table index -- so the decoder pops the index first
long encode(const Table& t, const int32_t* sym, size_t count, uint32_t* out, size_t cap, bool two_state_words = false, int shift = 0) {
    std::vector<uint32_t> rev;                                  // words in emission order; the message is this order REVERSED + state
    rev.reserve(count / 3 + 8);
    uint64_t state = 0;
    const int n = t.n();
    auto push = [&](uint32_t left, uint32_t prob) {
        if ((state >> (64 - PREC)) >= prob) { rev.push_back((uint32_t)state); state >>= 32; }
        state = ((state / prob) << PREC) | (state % prob + left);
    };
    for (size_t i = count; i-- > 0;) {
        if (sym[i] < 0) return -1;
        const int32_t s = sym[i] >> shift;
        if (s >= n) return -1;
        if (shift) push(((uint32_t)sym[i] & ((1u << shift) - 1u)) << (PREC - shift), 1u << (PREC - shift));
        push(t.cdf[(size_t)s], t.cdf[(size_t)s + 1] - t.cdf[(size_t)s]);
    }
    const size_t state_words = two_state_words ? 2 : state == 0 ? 0 : (state >> 32 ? 2 : 1);
    const size_t total = rev.size() + state_words;
    if (out == nullptr || cap < total) return (long)total;
    // layout: [bulk words in REVERSE emission order (= the order the decoder refills in), low state word, high state word]
    size_t w = 0;
    for (size_t i = rev.size(); i-- > 0;) out[w++] = rev[i];
    if (state_words >= 1) out[w++] = (uint32_t)state;
    if (state_words == 2) out[w++] = (uint32_t)(state >> 32);
    return (long)total;
}

int decode(const Table& t, const uint32_t* words, size_t n_words, size_t count, int32_t* sym) {
    // the state is the LAST one or two words; whether it has two is decided exactly as the encoder did: a two-word state has a
    // non-zero high word, and the encoder writes the high word last
    uint64_t state = 0;
    size_t bulk = n_words;
    // candidates are tried from two state words down; a wrong guess cannot pass the end check (all bulk words consumed, state 0)
    auto run = [&](size_t state_words) -> bool {
        if (state_words > n_words) return false;
        bulk = n_words - state_words;
        state = 0;
        if (state_words >= 1) state = words[bulk];
        if (state_words == 2) { if (words[bulk + 1] == 0) return false; state |= (uint64_t)words[bulk + 1] << 32; }
        if (state_words == 1 && state == 0) return false;
        size_t next = 0;
        for (size_t i = 0; i < count; ++i) {
            const uint32_t q = (uint32_t)(state & (TOTAL - 1));
            const size_t s = (size_t)(std::upper_bound(t.cdf.begin(), t.cdf.end(), q) - t.cdf.begin()) - 1;
            const uint32_t left = t.cdf[s], prob = t.cdf[s + 1] - left;
            sym[i] = (int32_t)s;
            state = (state >> PREC) * prob + (q - left);
            if ((state >> 32) == 0 && next < bulk) state = (state << 32) | words[next++];
        }
        return next == bulk && state == 0;
    };
    for (int sw = 2; sw >= 0; --sw)
        if (run((size_t)sw)) return BNERV_OK;
    return bnerv_set_error(BNERV_E_ARG, "ans_decode: the words do not decode to %zu symbols under this model", count);
}

// One run of the chunked layout: `n_words` words = bulk words + the final state as exactly two words, so the state's
// place is known and the run is decoded once.  The refill rule is decode()'s.  Reads words[0 .. n_words) only.
// shift > 0: after the table index, `shift` raw bits (encode()); a value above max_off -- past the range in a partial last bucket -- fails the run
bool decode_run(const Table& t, const uint32_t* words, size_t n_words, size_t count, int32_t* sym, int shift = 0, uint32_t max_off = 0xffffffffu) {
    if (n_words < 2) return false;
    const size_t bulk = n_words - 2;
    uint64_t state = (uint64_t)words[bulk] | ((uint64_t)words[bulk + 1] << 32);
    size_t next = 0;
    for (size_t i = 0; i < count; ++i) {
        const uint32_t q = (uint32_t)(state & (TOTAL - 1));
        const size_t s = (size_t)(std::upper_bound(t.cdf.begin(), t.cdf.end(), q) - t.cdf.begin()) - 1;
        const uint32_t left = t.cdf[s], prob = t.cdf[s + 1] - left;
        uint32_t off = (uint32_t)s;
        state = (state >> PREC) * prob + (q - left);
        if ((state >> 32) == 0 && next < bulk) state = (state << 32) | words[next++];
        if (shift) {
            const uint32_t r = (uint32_t)(state & (TOTAL - 1));
            off = (off << shift) | (r >> (PREC - shift));
            state = ((state >> PREC) << (PREC - shift)) | (r & ((1u << (PREC - shift)) - 1u));
            if ((state >> 32) == 0 && next < bulk) state = (state << 32) | words[next++];
        }
        if (off > max_off) return false;
        sym[i] = (int32_t)off;
    }
    return next == bulk && state == 0;
}

constexpr size_t MAX_RUN_WORDS = 65535;

// The two run entry points of either model share these: `what` names the caller in the messages.
long encode_runs(const Table& t, const char* what, const int32_t* symbols, size_t n, int32_t min_sym, int run, uint32_t* out_words, size_t cap_words,
                 unsigned short* out_run_words, int shift = 0, const int32_t* wide_max = nullptr) {
    const int32_t max_sym = wide_max ? *wide_max : min_sym + t.n() - 1;
    std::vector<int32_t> idx(n);
    for (size_t i = 0; i < n; ++i) {
        if (symbols[i] < min_sym || symbols[i] > max_sym) { bnerv_set_error(BNERV_E_ARG, "%s: symbol %d outside [%d, %d]", what, symbols[i], min_sym, max_sym); return -1; }
        idx[i] = symbols[i] - min_sym;
    }
    // every run through encode() from an empty state, its final state written as two words whatever its size
    std::vector<uint32_t> msg((size_t)run * (size_t)(PREC + shift) / 32 + 3);
    std::vector<uint32_t> all;
    all.reserve(n / 3 + 8);
    size_t k = 0;
    for (size_t at = 0; at < n; at += (size_t)run, ++k) {
        const size_t count = n - at < (size_t)run ? n - at : (size_t)run;
        const long got = encode(t, idx.data() + at, count, msg.data(), msg.size(), true, shift);
        if (got < 2 || (size_t)got > msg.size()) { bnerv_set_error(BNERV_E_ARG, "%s: run %zu takes %ld words (%zu at most)", what, k, got, msg.size()); return -1; }
        all.insert(all.end(), msg.begin(), msg.begin() + got);
        if (out_run_words) out_run_words[k] = (unsigned short)got;
    }
    if (out_words && cap_words >= all.size()) std::copy(all.begin(), all.end(), out_words);
    return (long)all.size();
}

int decode_runs(const Table& t, const char* what, const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                int32_t min_sym, int run, int32_t* symbols_out, int shift = 0, uint32_t max_off = 0xffffffffu) {
    size_t total = 0;
    for (size_t k = 0; k < n_runs; ++k) total += run_words[k];
    BNERV_REQUIRE(total == n_words, "%s: the run lengths add up to %zu words, the message has %zu", what, total, n_words);
    size_t at = 0;
    for (size_t k = 0; k < n_runs; ++k) {
        const size_t first = k * (size_t)run, count = n - first < (size_t)run ? n - first : (size_t)run;
        if (!decode_run(t, words + at, run_words[k], count, symbols_out + first, shift, max_off))
            return bnerv_set_error(BNERV_E_ARG, "%s: run %zu (%u words at word %zu) does not decode to %zu symbols under this model",
                                   what, k, (unsigned)run_words[k], at, count);
        for (size_t i = 0; i < count; ++i) symbols_out[first + i] += min_sym;
        at += run_words[k];
    }
    return BNERV_OK;
}

// The ONE place that turns a histogram into a table, integer arithmetic only: one slot per symbol, the other
// 2^24 - A split by floor((2^24 - A) * count / n), the slots lost to truncation (fewer than A) one each to the symbols in order of
// decreasing count, index order on ties.
bool counts_table(const uint32_t* counts, int A, Table& t) {
    if (!counts || A < 2 || A > (int)(TOTAL / 2)) return false;
    uint64_t n = 0;
    for (int k = 0; k < A; ++k) n += counts[k];
    if (n == 0) return false;
    const uint64_t free_slots = TOTAL - (uint32_t)A;
    std::vector<uint32_t> f((size_t)A);
    uint64_t used = 0;
    for (int k = 0; k < A; ++k) { f[(size_t)k] = 1u + (uint32_t)(free_slots * counts[k] / n); used += f[(size_t)k]; }
    std::vector<int> order((size_t)A);
    for (int k = 0; k < A; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] > counts[b]; });
    for (size_t j = 0; used < TOTAL; j = (j + 1) % (size_t)A) { ++f[(size_t)order[j]]; ++used; }
    t.cdf.resize((size_t)A + 1);
    t.cdf[0] = 0;
    for (int k = 0; k < A; ++k) t.cdf[(size_t)k + 1] = t.cdf[(size_t)k] + f[(size_t)k];
    return t.cdf[(size_t)A] == TOTAL;
}

// a caller's cumulative table: A + 1 entries from 0 to 2^24, strictly increasing
bool given_table(const uint32_t* cdf, int A, Table& t) {
    if (!cdf || A < 2 || A > (int)(TOTAL / 2) || cdf[0] != 0 || cdf[A] != TOTAL) return false;
    for (int k = 0; k < A; ++k)
        if (cdf[k + 1] <= cdf[k]) return false;
    t.cdf.assign(cdf, cdf + A + 1);
    return true;
}

}  // namespace

extern "C" long bnerv_ans_gaussian_cdf(int32_t min_sym, int32_t max_sym, double mean, double std_, uint32_t* out_cdf, size_t cap) {
    Table t;
    if (!gaussian_table(min_sym, max_sym, mean, std_, t)) { bnerv_set_error(BNERV_E_ARG, "ans_gaussian_cdf: bad model (min %d max %d mean %g std %g)", min_sym, max_sym, mean, std_); return -1; }
    if (out_cdf && cap >= t.cdf.size()) std::copy(t.cdf.begin(), t.cdf.end(), out_cdf);
    return (long)t.cdf.size();
}

extern "C" long bnerv_ans_counts_cdf(const uint32_t* counts, int A, uint32_t* out_cdf, size_t cap) {
    Table t;
    if (!counts_table(counts, A, t)) { bnerv_set_error(BNERV_E_ARG, "ans_counts_cdf: bad histogram (%d symbols, 2..%u, at least one counted)", A, TOTAL / 2); return -1; }
    if (out_cdf && cap >= t.cdf.size()) std::copy(t.cdf.begin(), t.cdf.end(), out_cdf);
    return (long)t.cdf.size();
}

extern "C" long bnerv_ans_encode_gaussian_runs(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std_, int run,
                                               uint32_t* out_words, size_t cap_words, unsigned short* out_run_words) {
    Table t;
    if (!symbols && n) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian_runs: null symbols"); return -1; }
    if (run < 1 || (size_t)run * PREC / 32 + 3 > MAX_RUN_WORDS) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian_runs: run = %d (a run's words must fit 16 bits)", run); return -1; }
    if (!gaussian_table(min_sym, max_sym, mean, std_, t)) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian_runs: bad model (min %d max %d mean %g std %g)", min_sym, max_sym, mean, std_); return -1; }
    return encode_runs(t, "ans_encode_gaussian_runs", symbols, n, min_sym, run, out_words, cap_words, out_run_words);
}

extern "C" int bnerv_ans_decode_gaussian_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                                              int32_t min_sym, int32_t max_sym, double mean, double std_, int run, int32_t* symbols_out) {
    Table t;
    BNERV_REQUIRE((words || !n_words) && (symbols_out || !n) && (run_words || !n_runs), "ans_decode_gaussian_runs: null buffer");
    BNERV_REQUIRE(run >= 1 && n_runs == (n + (size_t)run - 1) / (size_t)run, "ans_decode_gaussian_runs: %zu run lengths for %zu symbols in runs of %d", n_runs, n, run);
    BNERV_REQUIRE(gaussian_table(min_sym, max_sym, mean, std_, t), "ans_decode_gaussian_runs: bad model");
    return decode_runs(t, "ans_decode_gaussian_runs", words, n_words, run_words, n_runs, n, min_sym, run, symbols_out);
}

extern "C" long bnerv_ans_encode_table_runs(const int32_t* symbols, size_t n, int32_t min_sym, const uint32_t* cdf, int A, int run,
                                            uint32_t* out_words, size_t cap_words, unsigned short* out_run_words) {
    Table t;
    if (!symbols && n) { bnerv_set_error(BNERV_E_ARG, "ans_encode_table_runs: null symbols"); return -1; }
    if (run < 1 || (size_t)run * PREC / 32 + 3 > MAX_RUN_WORDS) { bnerv_set_error(BNERV_E_ARG, "ans_encode_table_runs: run = %d (a run's words must fit 16 bits)", run); return -1; }
    if (!given_table(cdf, A, t)) { bnerv_set_error(BNERV_E_ARG, "ans_encode_table_runs: bad table (%d symbols; strictly increasing from 0 to 2^24)", A); return -1; }
    return encode_runs(t, "ans_encode_table_runs", symbols, n, min_sym, run, out_words, cap_words, out_run_words);
}

extern "C" int bnerv_ans_decode_table_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                                           int32_t min_sym, const uint32_t* cdf, int A, int run, int32_t* symbols_out) {
    Table t;
    BNERV_REQUIRE((words || !n_words) && (symbols_out || !n) && (run_words || !n_runs), "ans_decode_table_runs: null buffer");
    BNERV_REQUIRE(run >= 1 && n_runs == (n + (size_t)run - 1) / (size_t)run, "ans_decode_table_runs: %zu run lengths for %zu symbols in runs of %d", n_runs, n, run);
    BNERV_REQUIRE(given_table(cdf, A, t), "ans_decode_table_runs: bad table (%d symbols; strictly increasing from 0 to 2^24)", A);
    return decode_runs(t, "ans_decode_table_runs", words, n_words, run_words, n_runs, n, min_sym, run, symbols_out);
}

// ---- wide runs: a table over the B buckets of 2^shift values, the low bits raw in the same state
namespace {
// B for [min_sym, max_sym] at `shift`, or 0 where the three do not go together
int wide_buckets(int32_t min_sym, int32_t max_sym, int shift) {
    if (max_sym < min_sym || shift < 0 || shift > BNERV_RANSW_MAX_SHIFT) return 0;
    const int64_t B = ((int64_t)max_sym - min_sym + ((int64_t)1 << shift)) >> shift;
    return B >= 2 && B <= (int64_t)(TOTAL / 2) && (int64_t)max_sym - min_sym < ((int64_t)1 << 28) ? (int)B : 0;
}
}  // namespace

extern "C" long bnerv_ans_gaussian_bucket_cdf(int32_t min_sym, int32_t max_sym, int shift, double mean, double std_, uint32_t* out_cdf, size_t cap) {
    Table t;
    if (shift < 0 || shift > BNERV_RANSW_MAX_SHIFT || !gaussian_table(min_sym, max_sym, mean, std_, t, shift)) {
        bnerv_set_error(BNERV_E_ARG, "ans_gaussian_bucket_cdf: bad model (min %d max %d shift %d mean %g std %g)", min_sym, max_sym, shift, mean, std_);
        return -1;
    }
    if (out_cdf && cap >= t.cdf.size()) std::copy(t.cdf.begin(), t.cdf.end(), out_cdf);
    return (long)t.cdf.size();
}

extern "C" long bnerv_ans_encode_wide_runs(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, const uint32_t* cdf, int B, int shift, int run,
                                           uint32_t* out_words, size_t cap_words, unsigned short* out_run_words) {
    Table t;
    if (!symbols && n) { bnerv_set_error(BNERV_E_ARG, "ans_encode_wide_runs: null symbols"); return -1; }
    if (B < 2 || wide_buckets(min_sym, max_sym, shift) != B) {
        bnerv_set_error(BNERV_E_ARG, "ans_encode_wide_runs: %d buckets for [%d, %d] at shift %d (0..%d)", B, min_sym, max_sym, shift, BNERV_RANSW_MAX_SHIFT);
        return -1;
    }
    if (run < 1 || (size_t)run * (size_t)(PREC + shift) / 32 + 3 > MAX_RUN_WORDS) { bnerv_set_error(BNERV_E_ARG, "ans_encode_wide_runs: run = %d (a run's words must fit 16 bits)", run); return -1; }
    if (!given_table(cdf, B, t)) { bnerv_set_error(BNERV_E_ARG, "ans_encode_wide_runs: bad table (%d buckets; strictly increasing from 0 to 2^24)", B); return -1; }
    return encode_runs(t, "ans_encode_wide_runs", symbols, n, min_sym, run, out_words, cap_words, out_run_words, shift, &max_sym);
}

extern "C" int bnerv_ans_decode_wide_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                                          int32_t min_sym, int32_t max_sym, const uint32_t* cdf, int B, int shift, int run, int32_t* symbols_out) {
    Table t;
    BNERV_REQUIRE((words || !n_words) && (symbols_out || !n) && (run_words || !n_runs), "ans_decode_wide_runs: null buffer");
    BNERV_REQUIRE(run >= 1 && n_runs == (n + (size_t)run - 1) / (size_t)run, "ans_decode_wide_runs: %zu run lengths for %zu symbols in runs of %d", n_runs, n, run);
    BNERV_REQUIRE(B >= 2 && wide_buckets(min_sym, max_sym, shift) == B, "ans_decode_wide_runs: %d buckets for [%d, %d] at shift %d (0..%d)", B, min_sym, max_sym, shift,
                  BNERV_RANSW_MAX_SHIFT);
    BNERV_REQUIRE(given_table(cdf, B, t), "ans_decode_wide_runs: bad table (%d buckets; strictly increasing from 0 to 2^24)", B);
    return decode_runs(t, "ans_decode_wide_runs", words, n_words, run_words, n_runs, n, min_sym, run, symbols_out, shift, (uint32_t)((int64_t)max_sym - min_sym));
}

extern "C" long bnerv_ans_encode_gaussian(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std_, uint32_t* out, size_t cap_words) {
    Table t;
    if (!symbols && n) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian: null symbols"); return -1; }
    if (!gaussian_table(min_sym, max_sym, mean, std_, t)) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian: bad model (min %d max %d mean %g std %g)", min_sym, max_sym, mean, std_); return -1; }
    std::vector<int32_t> idx(n);
    for (size_t i = 0; i < n; ++i) {
        if (symbols[i] < min_sym || symbols[i] > max_sym) { bnerv_set_error(BNERV_E_ARG, "ans_encode_gaussian: symbol %d outside [%d, %d]", symbols[i], min_sym, max_sym); return -1; }
        idx[i] = symbols[i] - min_sym;
    }
    return encode(t, idx.data(), n, out, cap_words);
}

extern "C" int bnerv_ans_decode_gaussian(const uint32_t* words, size_t n_words, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std_, int32_t* symbols_out) {
    Table t;
    BNERV_REQUIRE((words || !n_words) && (symbols_out || !n), "ans_decode_gaussian: null buffer");
    BNERV_REQUIRE(gaussian_table(min_sym, max_sym, mean, std_, t), "ans_decode_gaussian: bad model");
    const int rc = decode(t, words, n_words, n, symbols_out);
    if (rc != BNERV_OK) return rc;
    for (size_t i = 0; i < n; ++i) symbols_out[i] += min_sym;
    return BNERV_OK;
}

extern "C" long bnerv_ans_encode_categorical(const int32_t* symbols, size_t n, const double* probs, int K, uint32_t* out, size_t cap_words) {
    Table t;
    if ((!symbols && n) || !probs) { bnerv_set_error(BNERV_E_ARG, "ans_encode_categorical: null argument"); return -1; }
    if (!categorical_table(probs, K, t)) { bnerv_set_error(BNERV_E_ARG, "ans_encode_categorical: bad probabilities (K = %d)", K); return -1; }
    const long r = encode(t, symbols, n, out, cap_words);
    if (r < 0) bnerv_set_error(BNERV_E_ARG, "ans_encode_categorical: symbol outside [0, %d)", K);
    return r;
}

extern "C" int bnerv_ans_decode_categorical(const uint32_t* words, size_t n_words, size_t n, const double* probs, int K, int32_t* symbols_out) {
    Table t;
    BNERV_REQUIRE((words || !n_words) && (symbols_out || !n) && probs, "ans_decode_categorical: null argument");
    BNERV_REQUIRE(categorical_table(probs, K, t), "ans_decode_categorical: bad probabilities");
    return decode(t, words, n_words, n, symbols_out);
}
