"""Shared cases of the zstream tests (test_zstream_cpu.py, test_gpu_zstream.py): the five record shapes of qstream_cases pruned by magnitude,
a numpy restatement of the sparse de-quantisation, a pure-Python restatement of the zero parse, and a builder that turns host records into
a coded stream with the host coder.  A host record here is (uint8 symbols, bool keep, min, scale, outer, red, inner, flag)."""
import numpy as np
import torch

import qstream_cases as Q

F32, F16 = Q.F32, Q.F16
RUN, ZERO, LEAVES = 256, 256, 266
PARSES = ("single", "runs")

# (outer, red, inner, dtype flag) of the grid quant_tensor_sparse picks for the five tensors with 40 % of their entries pruned by magnitude
FIVE_SPARSE_GEOMETRIES = [(1, 12, 1, F32), (1, 64, 27, F16), (8, 64, 1, F16), (96, 60, 9, F16), (1, 60, 24, F16)]


def prune(t, sparsity):
    """`t` with its round(sparsity * numel) entries of smallest magnitude set to zero (ties by position)."""
    k = int(round(sparsity * t.numel()))
    out = t.clone().reshape(-1)
    if k:
        out[out.abs().argsort(stable=True)[:k]] = 0.0
    return out.reshape(t.shape)


def host_record(rec, geometry):
    outer, red, inner, flag = geometry
    return (rec["quant"].reshape(-1).numpy().copy(), rec["keep"].reshape(-1).numpy().copy(), rec["min"].reshape(-1).numpy().copy(),
            rec["scale"].reshape(-1).numpy().copy(), outer, red, inner, flag)


def five_sparse_records(sparsity=0.4):
    """-> [(host record, `rebuilt` of quant_tensor_sparse as a flat fp32 array, the pruned tensor)]; asserts the winning grids."""
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.hnerv_utils import quant_tensor_sparse
    out = []
    for t, want in zip(Q.five_tensors(), FIVE_SPARSE_GEOMETRIES):
        t = prune(t, sparsity)
        rec, rebuilt = quant_tensor_sparse(t, 8)
        assert codec._grid_geometry(rec) == want, (tuple(t.shape), codec._grid_geometry(rec), want)
        assert rebuilt.dtype == torch.float32 and torch.equal(rec["keep"], t != 0)
        out.append((host_record(rec, want), rebuilt.reshape(-1).numpy().copy(), t))
    return out


def restate(q, keep, lo, step, outer, red, inner):
    """keep ? float32(min[s]) + float32(scale[s]) * float32(q[i]) : +0.0 (qstream_cases.restate under the mask)."""
    return np.where(keep, Q.restate(q, lo, step, outer, red, inner), np.float32(0.0)).astype(np.float32)


def hand_record(n_or_geometry, flag, rng, keep, symbols=None):
    """qstream_cases.hand_record with a keep mask (an array, or the probability that an element is kept)."""
    q, lo, step, outer, red, inner, flag = Q.hand_record(n_or_geometry, flag, rng, symbols)
    kp = rng.random(q.size) < keep if np.isscalar(keep) else np.asarray(keep, dtype=bool)
    assert kp.size == q.size
    return (np.where(kp, q, 0).astype(np.uint8), kp, lo, step, outer, red, inner, flag)


def parse_leaves(q, keep, parse, run=RUN):
    """The leaves of one record, run by run, in plain Python: [[leaf, ...] per run]."""
    runs = []
    for i0 in range(0, len(q), run):
        leaves, z = [], 0

        def flush():
            if parse == "single":
                leaves.extend([ZERO] * z)
            else:
                leaves.extend(ZERO + k for k in range(8, -1, -1) if (z >> k) & 1)

        for s, k in zip(q[i0:i0 + run], keep[i0:i0 + run]):
            if k:
                flush()
                z = 0
                leaves.append(int(s))
            else:
                z += 1
        flush()
        runs.append(leaves)
    return runs


def histogram(records, parse):
    hist = np.zeros(LEAVES - 1, dtype=np.int64)
    for r in records:
        for leaves in parse_leaves(r[0], r[1], parse):
            np.add.at(hist, leaves, 1)
    return hist


def stream(records, parse=None, lengths=None):
    """Host records -> (words, lengths, [run_bits per record], parse): the code and the parse of codec.sparse_code over all elements (or the
    given ones), the host coder."""
    from boosting_nerv_amd import codec, zstream
    from boosting_nerv_amd.lib.entropy_model import huffz_encode
    symbols = np.concatenate([r[0] for r in records])
    keep = np.concatenate([r[1] for r in records])
    counts = [r[0].size for r in records]
    if lengths is None:
        chosen, lengths, _, _ = codec.sparse_code(symbols, keep, counts)
        if parse is None:
            parse = chosen
        elif parse != chosen:                               # the code of the other parse: its own histogram
            from boosting_nerv_amd.train_nerv_all import _huffman_depths
            hist = zstream.parse_histogram(symbols, keep, counts, parse)
            used = np.flatnonzero(hist)
            depths = _huffman_depths(hist[used].tolist())
            lengths = np.zeros(LEAVES, dtype=np.uint8)
            lengths[used], lengths[-1] = depths[:-1], depths[-1]
    words, run_bits = huffz_encode(symbols, keep, counts, lengths, parse, RUN)
    split, at = [], 0
    for n in counts:
        k = zstream.n_runs(n)
        split.append(run_bits[at:at + k])
        at += k
    assert at == run_bits.size
    return words, lengths, split, parse


def zrecords(records, split):
    from boosting_nerv_amd import zstream
    return [zstream.ZRecord(r[0].size, r[4], r[5], r[6], r[7], int(r[1].sum()), r[2], r[3], rb) for r, rb in zip(records, split)]
