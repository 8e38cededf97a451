"""Shared cases of the qstream tests (test_qstream_cpu.py, test_gpu_qstream.py): the five quant_tensor records the issue names, a
numpy restatement of the de-quantisation, and a builder that turns host records into a coded stream with the host coder."""
import numpy as np
import torch

F32, F16 = 0, 1


def five_tensors():
    """Seed 0, in this order: a per-tensor fp32 grid, an axis-0 grid, an axis-1 grid, a larger axis-1 grid, an embedding-shaped axis-0 grid."""
    torch.manual_seed(0)
    return [torch.randn(12), torch.randn(64, 3, 3, 3), torch.randn(8, 64, 1, 1) * torch.logspace(-2, 0, 8)[:, None, None, None],
            torch.randn(96, 60, 3, 3) * 0.05, torch.randn(60, 4, 2, 3)]


# (outer, red, inner, dtype flag) of the grid quant_tensor picks for each of them under seed 0
FIVE_GEOMETRIES = [(1, 12, 1, F32), (1, 64, 27, F16), (8, 64, 1, F16), (96, 60, 9, F16), (1, 60, 24, F16)]


def host_record(rec, geometry):
    """A quant_tensor record as plain arrays: (uint8 symbols, min, scale, outer, red, inner, flag)."""
    outer, red, inner, flag = geometry
    return (rec["quant"].reshape(-1).numpy().copy(), rec["min"].reshape(-1).numpy().copy(), rec["scale"].reshape(-1).numpy().copy(), outer, red, inner, flag)


def five_records():
    """-> [(host record, `rebuilt` of quant_tensor as a flat fp32 array)]; asserts the winning grids."""
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.hnerv_utils import quant_tensor
    out = []
    for t, want in zip(five_tensors(), FIVE_GEOMETRIES):
        rec, rebuilt = quant_tensor(t, 8)
        assert codec._grid_geometry(rec) == want, (tuple(t.shape), codec._grid_geometry(rec), want)
        assert rebuilt.dtype == torch.float32
        out.append((host_record(rec, want), rebuilt.reshape(-1).numpy().copy()))
    return out


def restate(q, lo, step, outer, red, inner):
    """out[i] = float32(min[s]) + float32(scale[s]) * float32(q[i]), s = (i // (red * inner)) * inner + i % inner: one fp32 product, one
    fp32 sum (numpy fuses nothing)."""
    i = np.arange(q.size, dtype=np.int64)
    s = (i // (red * inner)) * inner + i % inner
    prod = step.astype(np.float32)[s] * q.astype(np.float32)
    assert prod.dtype == np.float32
    return lo.astype(np.float32)[s] + prod


def hand_record(n_or_geometry, flag, rng, symbols=None):
    """A record with a random grid.  n_or_geometry: an element count (one pair) or (outer, red, inner)."""
    outer, red, inner = (1, n_or_geometry, 1) if isinstance(n_or_geometry, int) else n_or_geometry
    n = outer * red * inner
    dt = np.float16 if flag == F16 else np.float32
    q = rng.integers(0, 256, size=n).astype(np.uint8) if symbols is None else np.asarray(symbols, dtype=np.uint8)
    assert q.size == n
    lo = rng.normal(size=outer * inner).astype(dt)
    step = (rng.random(size=outer * inner) * 0.01 + 1e-4).astype(dt)
    return (q, lo, step, outer, red, inner, flag)


def stream(records, lengths=None):
    """Host records -> (words, lengths, [run_bits per record]): the code of codec.huffman_lengths over all symbols (or the given lengths),
    the host coder."""
    from boosting_nerv_amd import codec, qstream
    from boosting_nerv_amd.lib.entropy_model import huff_encode
    symbols = np.concatenate([r[0] for r in records])
    counts = [r[0].size for r in records]
    if lengths is None:
        lengths = codec.huffman_lengths(np.bincount(symbols, minlength=256))
    words, run_bits = huff_encode(symbols, counts, lengths, qstream.RUN)
    split, at = [], 0
    for n in counts:
        k = qstream.n_runs(n)
        split.append(run_bits[at:at + k])
        at += k
    assert at == run_bits.size
    return words, lengths, split


def qrecords(records, split):
    from boosting_nerv_amd import qstream
    return [qstream.QRecord(r[0].size, r[3], r[4], r[5], r[6], r[1], r[2], rb) for r, rb in zip(records, split)]


def depth16_symbols():
    """Symbol k 2^k times, k = 0..15, shuffled: 65 535 symbols whose rarest has a 16-bit code."""
    q = np.concatenate([np.full(2 ** k, 3 * k + 1, dtype=np.uint8) for k in range(16)])
    np.random.default_rng(4).shuffle(q)
    return q
