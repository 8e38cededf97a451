"""Shared cases of the pstream tests (test_pstream_cpu.py, test_gpu_pstream.py): constructed clips of 8-bit embedding codes, a builder that
turns one into a whole file with the host coder, and a numpy restatement of the chain and the de-quantisation."""
import struct
import zlib

import numpy as np

import qstream_cases as Q
import zstream_cases as Z

P = 576                                    # 4 x 12 x 12: two full runs of 256 symbols and one of 64
SHAPE = (4, 12, 12)
F32, F16 = Q.F32, Q.F16


def walk_clip(n, seed=1):
    """Frame 0 uniform over all 256 codes, every later frame the one before +-1 or unchanged, mod 256: some element steps from 255 to 0 and
    some from 0 to 255 (asserted).  A frame on its own costs about 8 bits a symbol, its differences under two: every t >= 1 is inter."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, P), dtype=np.uint8)
    q[0] = rng.integers(0, 256, size=P)
    for t in range(1, n):
        q[t] = q[t - 1] + rng.integers(-1, 2, size=P).astype(np.uint8)
    if n >= 8:
        assert ((q[:-1] == 255) & (q[1:] == 0)).any() and ((q[:-1] == 0) & (q[1:] == 255)).any()
    return q


def uniform_clip(n, seed=2):
    """Independent frames, uniform over the 64 codes of the default --quant_embed_bit 6.  A frame on its own costs 6 bits a symbol; the
    difference of two independent uniform codes is triangular over 127 values, about 6.7 bits: no frame is inter and the file has no inter table."""
    return np.random.default_rng(seed).integers(0, 64, size=(n, P)).astype(np.uint8)


def black_clip(n, cut, seed=3):
    """walk_clip with frame `cut` all zero -- a black frame: as differences to its neighbour it is as costly as a frame of uniform codes,
    on its own it is one symbol.  The frame after it is the walk again (its differences to a black frame are its own codes: either kind)."""
    q = walk_clip(n, seed)
    q[cut] = 0
    return q


def tiny_fallback_clip():
    """Two equal frames of 4 + 4 codes.  Frame 1 as differences is 8 one-bit symbols against 12 bits on its own, so step 2 of the rule says
    inter -- but two strings are two words where one string of 24 bits is one: step 4 falls back to all intra."""
    return np.array([[7, 7, 7, 7, 9, 9, 9, 9]] * 2, dtype=np.uint8)


def chain(sym, pred):
    """q_t = pred[t] ? (q_{t-1} + sym_t) mod 256 : sym_t."""
    q = np.array(sym, dtype=np.uint8)
    for t in range(1, q.shape[0]):
        if pred[t]:
            q[t] = q[t - 1] + sym[t]
    return q


def restate(q, lo, step, outer, red, inner):
    """float32(min[s]) + float32(scale[s]) * float32(q), s on the grid of the whole [N, P] tensor: Q.restate of the flat codes."""
    return Q.restate(q.reshape(-1), lo, step, outer, red, inner).reshape(q.shape)


def grid(n, count, axis, flag, rng, shape=None):
    """(lo, step, outer, red, inner) of a quant_tensor-shaped grid on an [N, *shape] tensor: axis None = one pair, axis k = reduced over axis k."""
    dims = (n,) + tuple(shape or (count,))
    assert int(np.prod(dims)) == n * count
    if axis is None:
        outer, red, inner = 1, n * count, 1
    else:
        outer, red, inner = int(np.prod(dims[:axis], dtype=np.int64)), dims[axis], int(np.prod(dims[axis + 1:], dtype=np.int64))
    dt = np.float16 if flag == F16 else np.float32
    return rng.normal(size=outer * inner).astype(dt), (rng.random(size=outer * inner) * 0.01 + 1e-4).astype(dt), outer, red, inner


def embeds_of(q, shape=SHAPE, flag=F32, seed=5):
    """The PEmbeds of the codes q [N, P] under one random (min, scale) pair: codec.code_embeds, the host path."""
    from boosting_nerv_amd import codec, pstream
    lo, step, outer, red, inner = grid(q.shape[0], q.shape[1], None, flag, np.random.default_rng(seed))
    return pstream.PEmbeds((q.shape[0],) + tuple(shape), outer, red, inner, flag, lo, step, *codec.code_embeds(q))


def tensor_section(sparse=False, seed=6):
    """Three hand-built tensor records coded by the host coder -> (settings, lengths, records, words, the module that frames them alone)."""
    from boosting_nerv_amd import qstream, zstream
    rng = np.random.default_rng(seed)
    settings = dict(model="HNeRV", huff_run=qstream.RUN, full_data_length=0, crop_list="180_320")
    if sparse:
        recs = [Z.hand_record(g, f, rng, k) for g, f, k in ((700, F32, 0.5), ((3, 50, 4), F16, 0.2), (5, F32, 0.9))]
        words, lengths, split, parse = Z.stream(recs)
        settings.update(zero_parse=parse, n_zero_leaves=int(Z.histogram(recs, parse)[zstream.ZERO:].sum()))
        return settings, lengths, Z.zrecords(recs, split), words, zstream
    recs = [Q.hand_record(g, f, rng) for g, f in ((700, F32), ((3, 50, 4), F16), (5, F32))]
    words, lengths, split = Q.stream(recs)
    return settings, lengths, Q.qrecords(recs, split), words, qstream


def file_of(q, sparse=False, shape=SHAPE):
    """A whole pstream file of the clip q with the tensor section of tensor_section() -> (bytes, settings, PEmbeds)."""
    from boosting_nerv_amd import pstream
    settings, lengths, records, words, _ = tensor_section(sparse)
    settings.update(full_data_length=int(q.shape[0]), embed_shape=[int(q.shape[0])] + list(shape), embed_pred=pstream.EMBED_PRED,
                    tensor_kind="sparse" if sparse else "dense")
    e = embeds_of(q, shape)
    return pstream.to_bytes(settings, lengths, records, words, e), settings, e


def frame(payload, magic=b"BNRP", version=1):
    """A payload in the container's framing, CRC computed here: how a damaged payload becomes a file whose CRC is right."""
    return struct.pack("<4sIQ", magic, version, len(payload)) + payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


def damaged(q, settings=None, sparse=False, **fields):
    """file_of(q) with the given PEmbeds fields (and / or settings) replaced and the CRC recomputed: no writer check is in the way."""
    from boosting_nerv_amd import pstream, qstream, zstream
    _, lengths, records, words, fmt = tensor_section(sparse)
    _, full, e = file_of(q, sparse)
    s = full if settings is None else settings
    payload = b"".join(qstream._header(s) + fmt._section(lengths, records, words) + pstream._embed_section(e._replace(**fields)))
    return frame(payload)
