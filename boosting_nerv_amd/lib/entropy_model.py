"""Rate model of the CEM compression path (reference lib/entropy_model.py:14-43, :100-114): bits of a code tensor under a
Gaussian fitted to it, with additive uniform noise while training and on the rounded symbols otherwise.

`real_bitrate` (reference: constriction's QuantizedGaussian + AnsCoder, lib/entropy_model.py:46-62) is the size of the message
the range-ANS coder of this build (csrc/ans.cpp behind bnerv_ans_encode_gaussian: same stream code and model construction as
constriction's defaults) produces for the rounded symbols -- a bitstream, not an estimate.  constriction itself is a third-party
dependency absent from the reference tree, so byte-for-byte equality with ITS stream is PARITY UNPINNED; the tests pin
decode(encode(x)) == x and the distance to the ideal code length."""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd import Function

from .. import _lib as L


class LowerBound(Function):                                   # lib/entropy_model.py:100-114
    @staticmethod
    def forward(ctx, inputs, bound):
        b = torch.ones_like(inputs) * bound
        ctx.save_for_backward(inputs, b)
        return torch.max(inputs, b)

    @staticmethod
    def backward(ctx, grad_output):
        inputs, b = ctx.saved_tensors
        pass_through = (inputs >= b) | (grad_output < 0)
        return pass_through.type(grad_output.dtype) * grad_output, None


def ideal_code_bits(quant, mean, std):
    """-sum log2 p(q) under the quantised Gaussian restricted to the support of the symbols (the lower bound of any coder)."""
    q = quant.detach().double().flatten().round()
    lo, hi = q.min(), q.max()
    if lo == hi:
        hi = lo + 1
    n = torch.distributions.normal.Normal(mean.detach().double(), std.detach().double().clamp(1e-5, 1e10))
    z = n.cdf(hi + 0.5) - n.cdf(lo - 0.5)
    p = (n.cdf(q + 0.5) - n.cdf(q - 0.5)) / z
    return float((-torch.log2(p.clamp_min(1e-300))).sum())


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ans_encode_gaussian(symbols, lo, hi, mean, std):
    """int32 symbols in [lo, hi] -> uint32 words of the rANS message (numpy)."""
    lib = L.load()
    sym = _i32(symbols)
    need = lib.bnerv_ans_encode_gaussian(sym.ctypes.data, sym.size, int(lo), int(hi), float(mean), float(std), None, 0)
    if need < 0:
        L.check(-1, "bnerv_ans_encode_gaussian")
    out = np.empty(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_ans_encode_gaussian(sym.ctypes.data, sym.size, int(lo), int(hi), float(mean), float(std), out.ctypes.data, out.size)
    assert got == need
    return out[:need]


def ans_decode_gaussian(words, n, lo, hi, mean, std):
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.empty(max(int(n), 1), dtype=np.int32)
    L.check(lib.bnerv_ans_decode_gaussian(w.ctypes.data, w.size, int(n), int(lo), int(hi), float(mean), float(std), out.ctypes.data), "bnerv_ans_decode_gaussian")
    return out[:n]


def ans_gaussian_cdf(lo, hi, mean, std):
    """The hi - lo + 2 cumulative 24-bit slot counts of the quantised Gaussian on [lo, hi] (uint32 numpy): the one table of the encoders,
    the host decoders and the device kernel (csrc/rans.hip)."""
    lib = L.load()
    need = lib.bnerv_ans_gaussian_cdf(int(lo), int(hi), float(mean), float(std), None, 0)
    if need < 0:
        L.check(-1, "bnerv_ans_gaussian_cdf")
    out = np.empty(need, dtype=np.uint32)
    assert lib.bnerv_ans_gaussian_cdf(int(lo), int(hi), float(mean), float(std), out.ctypes.data, out.size) == need
    return out


def ans_encode_gaussian_runs(symbols, lo, hi, mean, std, run):
    """int32 symbols in [lo, hi], cut into runs of `run` that are coded independently ->
    (uint32 words of all runs back to back, uint16 word count of every run: bulk words + two state words)."""
    lib = L.load()
    sym = _i32(symbols)
    run_words = np.zeros(max((sym.size + int(run) - 1) // max(int(run), 1), 1), dtype=np.uint16)
    args = (sym.ctypes.data, sym.size, int(lo), int(hi), float(mean), float(std), int(run))
    need = lib.bnerv_ans_encode_gaussian_runs(*args, None, 0, run_words.ctypes.data)
    if need < 0:
        L.check(-1, "bnerv_ans_encode_gaussian_runs")
    out = np.empty(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_ans_encode_gaussian_runs(*args, out.ctypes.data, out.size, run_words.ctypes.data)
    assert got == need
    return out[:need], run_words[:(sym.size + int(run) - 1) // int(run)]


def ans_decode_gaussian_runs(words, run_words, n, lo, hi, mean, std, run):
    """The inverse of ans_encode_gaussian_runs -> int32 symbols; raises BnervError naming the first run that does not consume exactly its
    words and end with state 0."""
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rw = np.ascontiguousarray(run_words, dtype=np.uint16)
    out = np.empty(max(int(n), 1), dtype=np.int32)
    L.check(lib.bnerv_ans_decode_gaussian_runs(w.ctypes.data, w.size, rw.ctypes.data, rw.size, int(n), int(lo), int(hi), float(mean), float(std), int(run),
                                               out.ctypes.data), "bnerv_ans_decode_gaussian_runs")
    return out[:n]


def ans_counts_cdf(counts):
    """The len(counts) + 1 cumulative 24-bit slot counts of a histogram (uint32 numpy): every symbol at least one slot,
    integer arithmetic only -- the one place a histogram becomes a table."""
    lib = L.load()
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.empty(c.size + 1, dtype=np.uint32)
    if lib.bnerv_ans_counts_cdf(c.ctypes.data, c.size, out.ctypes.data, out.size) != out.size:
        L.check(-1, "bnerv_ans_counts_cdf")
    return out


def ans_encode_table_runs(symbols, lo, cdf, run):
    """ans_encode_gaussian_runs under an explicit cumulative table: symbol lo + i owns [cdf[i], cdf[i + 1])."""
    lib = L.load()
    sym, t = _i32(symbols), np.ascontiguousarray(cdf, dtype=np.uint32)
    run_words = np.zeros(max((sym.size + int(run) - 1) // max(int(run), 1), 1), dtype=np.uint16)
    args = (sym.ctypes.data, sym.size, int(lo), t.ctypes.data, t.size - 1, int(run))
    need = lib.bnerv_ans_encode_table_runs(*args, None, 0, run_words.ctypes.data)
    if need < 0:
        L.check(-1, "bnerv_ans_encode_table_runs")
    out = np.empty(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_ans_encode_table_runs(*args, out.ctypes.data, out.size, run_words.ctypes.data)
    assert got == need
    return out[:need], run_words[:(sym.size + int(run) - 1) // int(run)]


def ans_decode_table_runs(words, run_words, n, lo, cdf, run):
    """The inverse of ans_encode_table_runs -> int32 symbols; raises BnervError naming the first run that does not decode."""
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rw = np.ascontiguousarray(run_words, dtype=np.uint16)
    t = np.ascontiguousarray(cdf, dtype=np.uint32)
    out = np.empty(max(int(n), 1), dtype=np.int32)
    L.check(lib.bnerv_ans_decode_table_runs(w.ctypes.data, w.size, rw.ctypes.data, rw.size, int(n), int(lo), t.ctypes.data, t.size - 1, int(run),
                                            out.ctypes.data), "bnerv_ans_decode_table_runs")
    return out[:n]


def ans_gaussian_bucket_cdf(lo, hi, shift, mean, std):
    """ans_gaussian_cdf over the ceil((hi - lo + 1) / 2^shift) buckets of 2^shift values from lo: bucket j starts at
    lo + j * 2^shift - 0.5, the last ends at hi + 0.5.  With shift 0 it is ans_gaussian_cdf entry for entry."""
    lib = L.load()
    need = lib.bnerv_ans_gaussian_bucket_cdf(int(lo), int(hi), int(shift), float(mean), float(std), None, 0)
    if need < 0:
        L.check(-1, "bnerv_ans_gaussian_bucket_cdf")
    out = np.empty(need, dtype=np.uint32)
    assert lib.bnerv_ans_gaussian_bucket_cdf(int(lo), int(hi), int(shift), float(mean), float(std), out.ctypes.data, out.size) == need
    return out


def ans_encode_wide_runs(symbols, lo, hi, cdf, shift, run):
    """ans_encode_table_runs for a range of any width: symbol - lo = (bucket << shift) | low, the bucket under `cdf` (one
    entry per bucket), low as `shift` raw bits in the same state.  A run takes at most run * (24 + shift) / 32 + 3 words."""
    lib = L.load()
    sym, t = _i32(symbols), np.ascontiguousarray(cdf, dtype=np.uint32)
    run_words = np.zeros(max((sym.size + int(run) - 1) // max(int(run), 1), 1), dtype=np.uint16)
    args = (sym.ctypes.data, sym.size, int(lo), int(hi), t.ctypes.data, t.size - 1, int(shift), int(run))
    need = lib.bnerv_ans_encode_wide_runs(*args, None, 0, run_words.ctypes.data)
    if need < 0:
        L.check(-1, "bnerv_ans_encode_wide_runs")
    out = np.empty(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_ans_encode_wide_runs(*args, out.ctypes.data, out.size, run_words.ctypes.data)
    assert got == need
    return out[:need], run_words[:(sym.size + int(run) - 1) // int(run)]


def ans_decode_wide_runs(words, run_words, n, lo, hi, cdf, shift, run):
    """The inverse of ans_encode_wide_runs -> int32 symbols; raises BnervError naming the first run that does not decode, a value above
    `hi` in the last bucket included."""
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rw = np.ascontiguousarray(run_words, dtype=np.uint16)
    t = np.ascontiguousarray(cdf, dtype=np.uint32)
    out = np.empty(max(int(n), 1), dtype=np.int32)
    L.check(lib.bnerv_ans_decode_wide_runs(w.ctypes.data, w.size, rw.ctypes.data, rw.size, int(n), int(lo), int(hi), t.ctypes.data, t.size - 1, int(shift),
                                           int(run), out.ctypes.data), "bnerv_ans_decode_wide_runs")
    return out[:n]


def ans_encode_categorical(symbols, probs):
    """symbols 0 .. K-1 under probs[K] -> uint32 words."""
    lib = L.load()
    sym = _i32(symbols)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    need = lib.bnerv_ans_encode_categorical(sym.ctypes.data, sym.size, p.ctypes.data, p.size, None, 0)
    if need < 0:
        L.check(-1, "bnerv_ans_encode_categorical")
    out = np.empty(max(need, 1), dtype=np.uint32)
    lib.bnerv_ans_encode_categorical(sym.ctypes.data, sym.size, p.ctypes.data, p.size, out.ctypes.data, out.size)
    return out[:need]


def ans_decode_categorical(words, n, probs):
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    out = np.empty(max(int(n), 1), dtype=np.int32)
    L.check(lib.bnerv_ans_decode_categorical(w.ctypes.data, w.size, int(n), p.ctypes.data, p.size, out.ctypes.data), "bnerv_ans_decode_categorical")
    return out[:n]


def huff_encode(symbols, counts, lengths, run=L.HUFF_RUN):
    """uint8 symbols of the items back to back (counts[k] each) under the canonical code of the 257 `lengths` ->
    (uint32 words of the bit string, uint16 bit length of every run of `run` symbols); csrc/huff.cpp, DESIGN section 26."""
    lib = L.load()
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    if ln.size != L.HUFF_LEAVES or int(cnt.sum()) != sym.size or run < 1:
        raise ValueError(f"huff_encode: need {L.HUFF_LEAVES} code lengths, counts that add up to the symbols and a positive run length")
    n_runs = int(sum((int(c) + run - 1) // run for c in cnt))
    run_bits = np.zeros(max(n_runs, 1), dtype=np.uint16)
    args = (sym.ctypes.data, cnt.ctypes.data, cnt.size, ln.ctypes.data, int(run))
    need = lib.bnerv_huff_encode(*args, None, 0, run_bits.ctypes.data, run_bits.size)
    if need < 0:
        L.check(-1, "bnerv_huff_encode")
    out = np.zeros(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_huff_encode(*args, out.ctypes.data, out.size, run_bits.ctypes.data, run_bits.size)
    assert got == need
    return out[:need], run_bits[:n_runs]


def huff_decode(words, run_bits, counts, lengths, run=L.HUFF_RUN):
    """The inverse of huff_encode -> uint8 symbols; raises BnervError when a run does not end on its recorded bit."""
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rb = np.ascontiguousarray(run_bits, dtype=np.uint16)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    if ln.size != L.HUFF_LEAVES:
        raise ValueError(f"huff_decode: need {L.HUFF_LEAVES} code lengths")
    out = np.zeros(max(int(cnt.sum()), 1), dtype=np.uint8)
    L.check(lib.bnerv_huff_decode(w.ctypes.data, w.size, rb.ctypes.data, rb.size, cnt.ctypes.data, cnt.size, ln.ctypes.data, int(run), out.ctypes.data),
            "bnerv_huff_decode")
    return out[:int(cnt.sum())]


def huffz_encode(symbols, keep, counts, lengths, parse, run=L.HUFF_RUN):
    """The sparse form of huff_encode (csrc/huffz.cpp): uint8 symbols and keep bytes of the items back to back under the
    canonical code of the 266 `lengths`, zeros written as zero-run leaves under parse "single" | "runs" (or BNERV_HUFFZ_SINGLE | _RUNS) ->
    (uint32 words of the bit string, uint16 bit length of every run of `run` ELEMENTS)."""
    lib = L.load()
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    kp = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    parse = {"single": L.HUFFZ_SINGLE, "runs": L.HUFFZ_RUNS}.get(parse, parse)
    if ln.size != L.HUFFZ_LEAVES or int(cnt.sum()) != sym.size or kp.size != sym.size or run < 1:
        raise ValueError(f"huffz_encode: need {L.HUFFZ_LEAVES} code lengths, counts that add up to the symbols, one keep byte per symbol and a positive run length")
    n_runs = int(sum((int(c) + run - 1) // run for c in cnt))
    run_bits = np.zeros(max(n_runs, 1), dtype=np.uint16)
    args = (sym.ctypes.data, kp.ctypes.data, cnt.ctypes.data, cnt.size, ln.ctypes.data, int(parse), int(run))
    need = lib.bnerv_huffz_encode(*args, None, 0, run_bits.ctypes.data, run_bits.size)
    if need < 0:
        L.check(-1, "bnerv_huffz_encode")
    out = np.zeros(max(need, 1), dtype=np.uint32)
    got = lib.bnerv_huffz_encode(*args, out.ctypes.data, out.size, run_bits.ctypes.data, run_bits.size)
    assert got == need
    return out[:need], run_bits[:n_runs]


def huffz_decode(words, run_bits, counts, lengths, run=L.HUFF_RUN):
    """The inverse of huffz_encode -> (uint8 symbols, bool keep); a zero element has symbol 0.  Raises BnervError when a run does not end on
    its recorded bit, decodes the EOF leaf, or holds a zero-run leaf that passes its element count."""
    lib = L.load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rb = np.ascontiguousarray(run_bits, dtype=np.uint16)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    if ln.size != L.HUFFZ_LEAVES:
        raise ValueError(f"huffz_decode: need {L.HUFFZ_LEAVES} code lengths")
    n = int(cnt.sum())
    out, kp = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    L.check(lib.bnerv_huffz_decode(w.ctypes.data, w.size, rb.ctypes.data, rb.size, cnt.ctypes.data, cnt.size, ln.ctypes.data, int(run), out.ctypes.data,
                                   kp.ctypes.data), "bnerv_huffz_decode")
    return out[:n], kp[:n].astype(bool)


def compress_matrix_flatten_gaussian_global(matrix, mean, std):
    """Bits of the rANS message of the integer tensor `matrix` under QuantizedGaussian(min, max, mean, std) -- the reference's
    function of the same name (lib/entropy_model.py:46-62), which returns 8 * bytes of constriction's compressed buffer."""
    mean = float(mean)
    std = float(torch.as_tensor(std).clamp(1e-5, 1e10))
    sym = matrix.detach().int().flatten().cpu().numpy()
    lo, hi = int(sym.min()), int(sym.max())
    if lo == hi:
        hi = lo + 1
    return int(ans_encode_gaussian(sym, lo, hi, mean, std).size) * 32


def compress_matrix_flatten_categorical(matrix):
    """(uint32 words, counts, unique values) of the flattened integer array under its own histogram (reference
    lib/entropy_model.py:65-81: np.unique -> Categorical -> AnsCoder)."""
    flat = np.asarray(matrix).reshape(-1)
    unique, inverse, counts = np.unique(flat, return_inverse=True, return_counts=True)
    words = ans_encode_categorical(inverse.astype(np.int32), counts.astype(np.float64) / counts.sum())
    return words, counts, unique


class DiffEntropyModel:
    def __init__(self, distribution="gaussian"):
        if distribution != "gaussian":
            raise NotImplementedError("only the Gaussian rate model of the recipes is built (lib/entropy_model.py:36-39 also has Laplace)")
        self.distribution = distribution
        self.noise_source = None          # tests: callable(code) -> U(-.5,.5) draw, so both sides of a comparison share the numbers

    def cal_bitrate(self, code, quant, training):
        return self.cal_global_bitrate(code, quant, training)

    def cal_global_bitrate(self, code, quant, training):
        mean = torch.mean(code)
        std = torch.std(code)
        if training:
            noise = self.noise_source(code) if self.noise_source is not None else torch.empty_like(code).uniform_(-0.5, 0.5)
            x = code + noise
            real_bits = 0
        else:
            x = quant
            real_bits = compress_matrix_flatten_gaussian_global(quant, mean, std)
        bits = torch.sum(self.get_bits(x, mean, std))
        return {"bitrate": bits, "mean": mean, "std": std, "real_bitrate": real_bits}

    def get_bits(self, x, mu, sigma):
        sigma = sigma.clamp(1e-5, 1e10)
        # validate_args=False: the default argument check reads a device flag on the host every call (a sync per step, and not
        # capturable in a graph); sigma is clamped positive just above, so the check cannot fail
        gaussian = torch.distributions.normal.Normal(mu, sigma, validate_args=False)
        probs = gaussian.cdf(x + 0.5) - gaussian.cdf(x - 0.5)
        bits = -1.0 * torch.log(probs + 1e-5) / math.log(2.0)
        return LowerBound.apply(bits, 0)
