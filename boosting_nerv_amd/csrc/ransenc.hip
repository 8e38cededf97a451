// ransenc.hip -- the encode kernels of the chunked CEM file with per-record tables (boosting_nerv_amd/estream.py, codec.encode(...,
// tables="empirical")): int32 symbols on the device -> their histograms, the range-ANS words of every run under any
// number of tables, and those words back to back as the file stores them.  Three launches; the host in between only builds tables from the
// counts and picks a model per record.  Plain HIP C++: the atomics are atomicAdd / atomicOr on LDS and global dwords.
//
// sym_hist     a block of 256 threads counts one slice of BNERV_HIST_SLICE symbols of ONE item in a private LDS histogram (at most 4096
//              bins, 16 KiB) and adds the non-zero bins to the item's global counts: one global atomic per (block, used symbol) instead of
//              one per symbol.
// rans_encode  the decoder's block shape (csrc/rans.hip): one wave, up to 64 consecutive runs of ONE item, that item's cumulative table
//              in LDS.  Lane k encodes run k from its last symbol to its first with encode()'s arithmetic of csrc/ans.cpp, word for word:
//              64-bit state, a word leaves when (state >> 40) >= prob, state = ((state / prob) << 24) | (state % prob + left).  The symbols
//              reach the lanes through LDS, 64 per run and round, read from memory with consecutive lanes on consecutive elements; the
//              rounds go from the run's end to its start.  A lane stores its words from the END of its run's slot downwards, so the slot's
//              tail reads in file order: bulk words in refill order (the reverse of emission), state low, state high.
// rans_compact one wave per run copies the tail of a slot to its place in the output.
// Every index that comes from a descriptor is checked against the array it points into before it is used; a lane never stores outside its
// slot, a copy never outside `out`.
#include "common.h"

namespace {

constexpr int WAVE = 64, CH = 64, STRIDE = CH + 2, MAX_A = BNERV_RANS_MAX_ALPHABET, PREC = 24, HIST_THREADS = 256;
constexpr unsigned BAD = 0xffffu;                    // a staged symbol outside the table (table indices stay below 4096)

__global__ __launch_bounds__(HIST_THREADS) void sym_hist_kernel(const bnerv_hist_item* __restrict__ items, const unsigned n_items,
                                                                const unsigned* __restrict__ blocks, unsigned* __restrict__ counts,
                                                                const unsigned n_counts, int* __restrict__ err) {
    __shared__ unsigned hist[MAX_A];
    const unsigned item = blocks[2 * blockIdx.x], first = blocks[2 * blockIdx.x + 1];
    bool ok = item < n_items;
    bnerv_hist_item it = {};
    if (ok) it = items[item];
    const unsigned A = it.alphabet;
    ok = ok && it.sym != nullptr && A >= 1u && A <= (unsigned)MAX_A && it.out <= n_counts && A <= n_counts - it.out && first < it.n;
    if (!ok) {
        if (threadIdx.x == 0) atomicOr(err, 2);
        return;
    }
    for (unsigned i = threadIdx.x; i < A; i += HIST_THREADS) hist[i] = 0;
    __syncthreads();
    const unsigned end = it.n - first < (unsigned)BNERV_HIST_SLICE ? it.n : first + (unsigned)BNERV_HIST_SLICE;
    bool bad = false;
    for (unsigned i = first + threadIdx.x; i < end; i += HIST_THREADS) {
        const unsigned s = (unsigned)(it.sym[i] - it.lo);            // (wraps for a symbol below lo: then s >= A as well)
        if (s < A) atomicAdd(&hist[s], 1u);
        else bad = true;
    }
    if (bad) atomicOr(err, 1);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < A; i += HIST_THREADS)
        if (hist[i]) atomicAdd(&counts[it.out + i], hist[i]);
}

__global__ __launch_bounds__(WAVE) void rans_encode_kernel(const bnerv_rans_block* __restrict__ blocks, const bnerv_renc_item* __restrict__ items,
                                                           const unsigned n_items, const unsigned* __restrict__ tables, const unsigned n_table_words,
                                                           const unsigned run, unsigned* __restrict__ slots, const unsigned n_slots,
                                                           unsigned short* __restrict__ run_words, int* __restrict__ err) {
    __shared__ unsigned cdf[MAX_A + 1];
    __shared__ unsigned short stage[WAVE * STRIDE];      // run rr's symbols at rr * STRIDE: 33 dwords apart, so the lanes' reads hit 32 banks
    const unsigned lane = threadIdx.x;
    // ---- the block's descriptors, all uniform; anything that points outside the uploaded arrays ends the block before a dependent access
    const bnerv_rans_block b = blocks[blockIdx.x];
    bool ok = b.item < n_items;
    bnerv_renc_item it = {};
    if (ok) it = items[b.item];
    const unsigned A = it.alphabet;
    const unsigned item_runs = ok && it.n ? (it.n - 1u) / run + 1u : 0u;
    ok = ok && it.sym != nullptr && A >= 2u && A <= (unsigned)MAX_A && it.table <= n_table_words && A + 1u <= n_table_words - it.table && b.first < item_runs;
    const unsigned live = ok ? (item_runs - b.first < (unsigned)WAVE ? item_runs - b.first : (unsigned)WAVE) : 0u;
    ok = ok && b.run <= n_slots && live <= n_slots - b.run;
    if (!ok) {
        if (lane == 0) atomicOr(err, 2);
        return;
    }
    for (unsigned i = lane; i <= A; i += WAVE) cdf[i] = tables[it.table + i];

    // ---- lane k: run b.first + k of the item, slot b.run + k
    const unsigned S = run * PREC / 32 + 3;                                // the host's bound on a run's words
    const bool active = lane < live;
    const unsigned first_elem = (b.first + lane) * run;                   // (< it.n < 2^31 for an active lane)
    const unsigned cnt = active ? (it.n - first_elem < run ? it.n - first_elem : run) : 0u;
    unsigned* const slot = slots + (size_t)(b.run + (active ? lane : 0u)) * S;
    unsigned p = S - 2;                                                   // the next word goes to slot[--p]; slot[S - 2], slot[S - 1]: the state
    bool dead = false;
    unsigned long long state = 0;
    const unsigned block_cnt = it.n - b.first * run < run ? it.n - b.first * run : run;      // lane 0's count: no lane has more
    for (unsigned r = (block_cnt + CH - 1) / CH; r-- > 0;) {
        __syncthreads();                                                  // (the table on the first pass, the last round's reads after)
        const unsigned e = r * CH + lane;
        for (unsigned rr = 0; rr < live; ++rr) {
            const unsigned f = (b.first + rr) * run, c = it.n - f < run ? it.n - f : run;
            if (e < c) {
                const unsigned s = (unsigned)(it.sym[(size_t)f + e] - it.lo);
                stage[rr * STRIDE + lane] = (unsigned short)(s < A ? s : BAD);
            }
        }
        __syncthreads();
        const unsigned have = cnt > r * CH ? (cnt - r * CH < (unsigned)CH ? cnt - r * CH : (unsigned)CH) : 0u;
        for (unsigned k = have; k-- > 0;) {
            const unsigned s = stage[lane * STRIDE + k];
            if (dead) continue;
            if (s == BAD) { dead = true; continue; }
            const unsigned left = cdf[s], prob = cdf[s + 1] - left;
            if ((state >> (64 - PREC)) >= prob) {
                if (p == 0) { dead = true; continue; }                    // the word would leave the slot
                slot[--p] = (unsigned)state;
                state >>= 32;
            }
            state = ((state / prob) << PREC) | (state % prob + left);
        }
    }
    if (active) {
        if (dead) {
            atomicOr(err, 1);
            run_words[b.run + lane] = 0;
        } else {
            slot[S - 2] = (unsigned)state;
            slot[S - 1] = (unsigned)(state >> 32);
            run_words[b.run + lane] = (unsigned short)(S - p);
        }
    }
}

__global__ __launch_bounds__(WAVE) void rans_compact_kernel(const unsigned* __restrict__ slots, const unsigned n_slots, const unsigned S,
                                                            const bnerv_rans_copy* __restrict__ copies, unsigned* __restrict__ out, const unsigned n_out,
                                                            int* __restrict__ err) {
    const bnerv_rans_copy c = copies[blockIdx.x];
    if (c.slot >= n_slots || c.count > S || c.dst > n_out || c.count > n_out - c.dst) {
        if (threadIdx.x == 0) atomicOr(err, 2);
        return;
    }
    const unsigned* src = slots + (size_t)c.slot * S + (S - c.count);
    for (unsigned i = threadIdx.x; i < c.count; i += WAVE) out[c.dst + i] = src[i];
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int bnerv_sym_hist(void* stream, const bnerv_hist_item* items, int n_items, const uint32_t* blocks, size_t n_blocks, uint32_t* counts,
                              size_t n_counts, int* err) {
    BNERV_REQUIRE(items && blocks && counts && err, "sym_hist: null args");
    BNERV_REQUIRE(n_items > 0 && n_blocks > 0 && n_blocks <= 0x7fffffffu && n_counts > 0 && n_counts <= 0xffffffffu, "sym_hist: n_items=%d n_blocks=%zu n_counts=%zu",
                  n_items, n_blocks, n_counts);
    BNERV_REQUIRE(aligned(items, 8) && aligned(blocks, 4) && aligned(counts, 4) && aligned(err, 4), "sym_hist: items (8 bytes) / blocks / counts / err (4) are not aligned");
    hipLaunchKernelGGL(sym_hist_kernel, dim3((unsigned)n_blocks), dim3(HIST_THREADS), 0, reinterpret_cast<hipStream_t>(stream), items, (unsigned)n_items,
                       reinterpret_cast<const unsigned*>(blocks), reinterpret_cast<unsigned*>(counts), (unsigned)n_counts, err);
    BNERV_LAUNCH_CHECK("sym_hist");
    return BNERV_OK;
}

extern "C" int bnerv_rans_encode(void* stream, const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_renc_item* items, int n_items,
                                 const uint32_t* tables, size_t n_table_words, int run, uint32_t* slots, size_t n_slots, unsigned short* run_words, int* err) {
    BNERV_REQUIRE(blocks && items && tables && slots && run_words && err, "rans_encode: null args");
    BNERV_REQUIRE(run >= BNERV_RANS_MIN_RUN && run <= BNERV_RANS_MAX_RUN && run % WAVE == 0, "rans_encode: run = %d (a multiple of %d in %d..%d)", run, WAVE,
                  BNERV_RANS_MIN_RUN, BNERV_RANS_MAX_RUN);
    BNERV_REQUIRE(n_slots > 0 && n_slots < 0x7fffffffu && n_blocks > 0 && n_blocks <= 0x7fffffffu && n_items > 0 && n_table_words >= 3 && n_table_words <= 0xffffffffu,
                  "rans_encode: n_slots=%zu n_blocks=%zu n_items=%d n_table_words=%zu", n_slots, n_blocks, n_items, n_table_words);
    BNERV_REQUIRE(aligned(blocks, 16) && aligned(items, 8) && aligned(tables, 4) && aligned(slots, 4) && aligned(run_words, 2) && aligned(err, 4),
                  "rans_encode: blocks (16 bytes) / items (8) / tables / slots / err (4) / run_words (2) are not aligned");
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)n_blocks), dim3(WAVE), 0, reinterpret_cast<hipStream_t>(stream), blocks, items, (unsigned)n_items,
                       reinterpret_cast<const unsigned*>(tables), (unsigned)n_table_words, (unsigned)run, reinterpret_cast<unsigned*>(slots), (unsigned)n_slots,
                       run_words, err);
    BNERV_LAUNCH_CHECK("rans_encode");
    return BNERV_OK;
}

extern "C" int bnerv_rans_compact(void* stream, const uint32_t* slots, size_t n_slots, int slot_words, const bnerv_rans_copy* copies, size_t n_copies,
                                  uint32_t* out, size_t n_out, int* err) {
    BNERV_REQUIRE(slots && copies && out && err, "rans_compact: null args");
    BNERV_REQUIRE(n_slots > 0 && n_slots < 0x7fffffffu && slot_words >= 3 && n_copies > 0 && n_copies <= 0x7fffffffu && n_out > 0 && n_out <= 0xffffffffu,
                  "rans_compact: n_slots=%zu slot_words=%d n_copies=%zu n_out=%zu", n_slots, slot_words, n_copies, n_out);
    BNERV_REQUIRE(aligned(slots, 4) && aligned(copies, 16) && aligned(out, 4) && aligned(err, 4), "rans_compact: slots / out / err (4 bytes) / copies (16) are not aligned");
    hipLaunchKernelGGL(rans_compact_kernel, dim3((unsigned)n_copies), dim3(WAVE), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const unsigned*>(slots),
                       (unsigned)n_slots, (unsigned)slot_words, copies, reinterpret_cast<unsigned*>(out), (unsigned)n_out, err);
    BNERV_LAUNCH_CHECK("rans_compact");
    return BNERV_OK;
}
