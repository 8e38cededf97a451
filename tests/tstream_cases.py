"""Shared by tests/test_tstream_cpu.py and tests/test_gpu_tstream.py: clips of constructed embedding symbols whose
frames the choice rule must code in a known way, as hand-built version-1 files, and the numpy restatements the tests compare against.
Everything here is host code.  The patterns named below are conditions on the inputs: they were confirmed with the host coder when the
cases were written, at run 64 and 256 under both tables."""
import numpy as np

from wstream_cases import SETTINGS

EMBED_SHAPE = (4, 9, 16)
P = 4 * 9 * 16                                             # 576 symbols per frame
N_FRAMES = 6
RUNS = (64, 256)
TABLES = ("gaussian", "empirical")
FAR = (1 << 20) + 5                                        # a difference past the eligibility limit of 2^20


def walk(seed=3, n=N_FRAMES):
    """(a) a +-1 random walk from a uniform 8-bit frame: the differences take two values, every frame t >= 1 is inter."""
    rng = np.random.default_rng(seed)
    q = [rng.integers(0, 256, size=P)]
    for _ in range(n - 1):
        q.append(q[-1] + rng.choice((-1, 1), size=P))
    return np.stack(q).astype(np.int32)


def independent(seed=4, n=N_FRAMES):
    """(b) independent uniform 8-bit frames: a difference spans twice the range, every frame is intra."""
    return np.random.default_rng(seed).integers(0, 256, size=(n, P)).astype(np.int32)


def walk_with_black_frame():
    """(c) the walk with frame 3 all zeros: a constant record costs two state words per run, its difference a full frame -- frame 3 is intra."""
    q = walk()
    q[3] = 0
    return q


def walk_with_far_frame():
    """(d) the walk with frames 2.. moved up by 2^20 + 5: the difference record of frame 2 would be cheap (a near-constant) but lies past
    2^20, so it is not eligible and the frame is intra."""
    q = walk()
    q[2:] += FAR
    return q


CASES = {"walk": walk, "independent": independent, "black": walk_with_black_frame, "far": walk_with_far_frame}
MODES = {"walk": [0, 1, 1, 1, 1, 1], "independent": [0] * 6, "black": {1: 1, 2: 1, 3: 0}, "far": {1: 1, 2: 0, 3: 1}}      # frame -> pred that must hold


def version1_blob(q, seed=7):
    """A hand-built version-1 file, coded as codec.encode codes it -> bytes: a 700-symbol weight record, a constant bias record and one
    embedding record per row of q (scale 0.5, one beta for the clip, the Gaussian of the row's own float moments)."""
    from boosting_nerv_amd import bitstream
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(seed)

    def rec(sym, scale, beta=None):
        lo, hi = int(sym.min()), int(sym.max())
        hi = hi if hi > lo else lo + 1
        mean, std = float(np.float32(sym.mean())), float(np.float32(max(sym.std(), 1e-5)))
        return bitstream.Record(sym.size, np.float32(scale), np.float32(mean), np.float32(std), lo, hi, em.ans_encode_gaussian(sym, lo, hi, mean, std), beta)

    tensors = [rec(np.rint(rng.normal(0.0, 6.0, size=700)).astype(np.int32), 0.02), rec(np.full(12, -3, np.int32), 0.5)]
    beta = np.float32(-0.37)
    embeds = [rec(np.ascontiguousarray(row), 0.5, beta) for row in q]
    raw = [rng.normal(size=9).astype(np.float32)]
    return bitstream.to_bytes(dict(SETTINGS, full_data_length=len(q)), tensors, embeds, EMBED_SHAPE, raw)


def hand_built(held, preds, run=64):
    """A temporal file written record by record -> bytes: held[t] are the symbols record t holds (the frame, or its differences), each under the
    Gaussian of its integer moments; one 12-symbol tensor record in front."""
    from boosting_nerv_amd import tstream, wstream
    from boosting_nerv_amd.lib import entropy_model as em
    words = []

    def rec(sym, beta=None):
        sym = np.ascontiguousarray(sym, dtype=np.int32)
        lo, hi = int(sym.min()), max(int(sym.max()), int(sym.min()) + 1)
        shift = wstream.min_shift(lo, hi)
        mean, std = tstream.delta_moments(*tstream.delta_sums(sym))
        w, rw = em.ans_encode_wide_runs(sym, lo, hi, em.ans_gaussian_bucket_cdf(lo, hi, shift, float(mean), float(std)), shift, run)
        words.append(w)
        return wstream.WRecord(sym.size, np.float32(0.5), lo, hi, 0, shift, mean, std, None, rw, beta)

    tensors = [rec(np.arange(12) - 6)]
    embeds = [rec(h, np.float32(0.25)) for h in held]
    settings = dict(SETTINGS, full_data_length=len(held), ans_run=run, ans_tables="gaussian", ans_wide=True, embed_pred="prev")
    return tstream.to_bytes(settings, tensors, embeds, preds, EMBED_SHAPE, [], np.concatenate(words))


SIDE_ITEMS = ("ans_words", "tables", "tensor_side", "embed_side")


def check_bound(temporal_budget, wide_budget):
    """The consequence of the choice rule: words, tables and side of the temporal file are at most those of the wide file of the same run and
    tables plus the pred byte of every frame."""
    t, w = (sum(b[k] for k in SIDE_ITEMS) for b in (temporal_budget, wide_budget))
    assert t <= w + 8 * temporal_budget["n_embeds"], (t, w, temporal_budget["n_embeds"])
    assert temporal_budget["run_index"] == wide_budget["run_index"] and temporal_budget["raw"] == wide_budget["raw"]


def delta_reference(q):
    """int64 / uint64 numpy restatement of ops.EmbedDelta on an int32 [N, P] array -> (d, lo, hi, s1, s2); row 0 of all is zero."""
    q = np.asarray(q, dtype=np.int64)
    d = np.zeros_like(q)
    d[1:] = q[1:] - q[:-1]
    du = d.astype(np.uint64)                                # two's complement: the square mod 2^64 is the square of the wrapped value
    s2 = (du * du).sum(axis=1, dtype=np.uint64)
    return d, d.min(axis=1), d.max(axis=1), d.sum(axis=1, dtype=np.int64), s2


def chain_reference(sym, pred, scale, beta):
    """numpy restatement of ops.EmbedChainDequant: the chain in int64, then np.float32(q) * scale + beta as two float32 operations."""
    q = np.zeros(sym.shape, dtype=np.int64)
    for t in range(sym.shape[0]):
        q[t] = (q[t - 1] if t and pred[t] else 0) + sym[t]
    scale, beta = (np.asarray(v, dtype=np.float32).reshape(-1, 1) for v in (scale, beta))
    return q, (q.astype(np.int32).astype(np.float32) * scale).astype(np.float32) + beta
