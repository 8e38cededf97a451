"""Container of a compressed video whose frame embeddings are coded with knowledge of the frame before: the wide chunked
CEM file of wstream.py in which the embedding record of frame t >= 1 holds either the frame's symbols q_t (intra: exactly the wstream
record) or the integer differences d_t = q_t - q_{t-1} (inter), whichever the encoder found cheaper.  ScaleBeta_T has one learnt (scale,
beta) for the clip, so the symbols of all frames lie on one integer grid and the difference is exact: nothing is lost.

Host-only code (numpy and struct), little-endian throughout; the framing is container.py's, the payload rstream.py's and the records
wstream.py's: this kind is wstream.KIND with a magic and a settings check of its own and a lead byte:

    magic "BNRT" | version u32 (1) | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: a wstream header -- "ans_wide": true stays -- plus "embed_pred": "prev")
                n_tensors u32 | n_tensors x record
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (pred u8 | record | beta f32)
                n_raw u32 | n_raw x (count u32 | count x f32)
                n_words u32 | n_words x u32
    pred 0: the record's symbols are q_t;  pred 1: they are d_t, and q_t = q_{t-1} + d_t.

A record that holds differences is an ordinary wstream record: range, shift, Gaussian or table of its own.  Its Gaussian comes from
delta_moments() -- exact integer sums, so the device path and the host path of the encoder cannot differ.

read() raises ValueError wherever wstream.read does, and for a pred byte above 1, pred 1 on frame 0, an embedding record whose count is not
C * h * w, a header without "embed_pred": "prev", and a file without embedding records (nothing to predict: write the wide kind).  info()
books every bit under estream's eight items; the pred byte counts as embedding side."""
import math
from collections import namedtuple

import numpy as np

from . import container, rstream, wstream
from .estream import ITEMS      # noqa: F401  (re-exported)

MAGIC = b"BNRT"
VERSION = 1
EMBED_PRED = "prev"
INTRA, INTER = 0, 1
MAX_DELTA = 1 << 20                        # an inter record is eligible when every |d| <= 2^20 ...
MAX_COUNT = 1 << 24                        # ... and C * h * w <= 2^24: sum d^2 <= 2^64, the span far below the wide kind's 2^28

TStream = namedtuple("TStream", "settings tensors embeds preds embed_shape raw words")
TStream.__doc__ = """settings: dict (a wstream header plus "embed_pred");  tensors / embeds: [WRecord];  preds: [0 | 1], one per embedding record;
embed_shape: (C, h, w);  raw: [float32 array];  words: uint32 array, every run of every record (tensors, then embeds) back to back"""


def _check_settings(who, settings):
    run = wstream._check_settings(who, settings)
    if settings.get("embed_pred") != EMBED_PRED:
        raise ValueError(f'{who}: the header\'s "embed_pred" is {settings.get("embed_pred")!r} (this kind says {EMBED_PRED!r})')
    return run


def _check_embeds(who, embeds, preds, embed_shape):
    if not embeds:
        raise ValueError(f"{who}: no embedding records (a model without frame embeddings has nothing to predict: write the wide kind)")
    if len(preds) != len(embeds):
        raise ValueError(f"{who}: {len(preds)} pred bytes for {len(embeds)} embedding records")
    count = int(np.prod(embed_shape, dtype=np.int64))
    for k, (r, p) in enumerate(zip(embeds, preds)):
        if p not in (INTRA, INTER):
            raise ValueError(f"{who}: the pred byte of frame {k} is {p} (0: intra, 1: the frame before)")
        if p == INTER and k == 0:
            raise ValueError(f"{who}: frame 0 is predicted (pred 1): there is no frame before it")
        if r.count != count:
            raise ValueError(f"{who}: the embedding record of frame {k} has {r.count} symbols, the embedding shape {tuple(embed_shape)} has {count}")


KIND = wstream.KIND._replace(who="tstream", magic=MAGIC, check_settings=_check_settings, lead=True)


def to_bytes(settings, tensors, embeds, preds, embed_shape, raw=(), words=()):
    embeds, preds = list(embeds), [int(p) for p in preds]
    if embeds and embed_shape is None:
        raise ValueError("tstream.write: embedding records need embed_shape (C, h, w)")
    _check_embeds("tstream.write", embeds, preds, embed_shape if embeds else (0,))
    return container.frame(MAGIC, VERSION, rstream.payload(KIND, settings, list(tensors), embeds, embed_shape, list(raw), words, preds))


def write(path_or_buffer, settings, tensors, embeds, preds, embed_shape, raw=(), words=()):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, tensors, embeds, preds, embed_shape, raw, words))


def _parse(path_or_buffer):
    (settings, tensors, embeds, embed_shape, raw, words), bits, nbytes, preds = rstream.parse(KIND, path_or_buffer)
    _check_embeds("tstream", embeds, preds, embed_shape if embeds else (0,))
    return TStream(settings, tensors, embeds, preds, embed_shape, raw, words), bits, nbytes


def read(path_or_buffer):
    """-> TStream(settings, tensors, embeds, preds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits, under estream.info's eight items (the pred byte of a frame counts as embedding side) -- plus "total" =
    their sum = 8 * file size, wstream.info's counts, "n_inter_frames" and "n_intra_frames"."""
    ts, bits, nbytes = _parse(path_or_buffer)
    out = wstream._budget(ts, bits, nbytes)
    out.update(embed_pred=ts.settings["embed_pred"], n_inter_frames=int(sum(p == INTER for p in ts.preds)), n_intra_frames=int(sum(p == INTRA for p in ts.preds)))
    return out


def decode_record(ts, k):
    """The symbols record k (tensors, then embeds) holds, decoded on the host (int32 numpy): for an inter record the differences."""
    return wstream.decode_record(ts, k)


def decode_embeds(ts):
    """The host oracle of the decoder's chain: the int32 [N, C*h*w] symbols q of every frame, q_t = q_{t-1} + d_t where frame t is predicted.
    Raises ValueError for a chain that leaves int32."""
    rows, q = [], None
    for k, p in enumerate(ts.preds):
        s = decode_record(ts, len(ts.tensors) + k).astype(np.int64)
        q = q + s if p == INTER else s
        if int(q.min()) < -(1 << 31) or int(q.max()) >= 1 << 31:
            raise ValueError(f"tstream: the chain of frame {k} leaves int32")
        rows.append(q)
    return np.stack(rows).astype(np.int32)


def delta_sums(d):
    """(n, s1, s2) of a difference record as the device counts them: s1 = sum d, s2 = sum d^2 mod 2^64 (exact while n * max d^2 < 2^64)."""
    d = np.asarray(d).astype(np.int64).reshape(-1)
    return int(d.size), int(d.sum(dtype=np.int64)), int((d * d).astype(np.uint64).sum(dtype=np.uint64))


def delta_moments(n, s1, s2):
    """The Gaussian of an inter record, the ONE place it comes from: mean = float32(s1 / n), std = float32(sqrt((n s2 - s1^2) / (n (n - 1))))
    (the unbiased one, as torch.std; 0 for n == 1), Python integers into the true division, then the clamp of the version-1 coder to
    [1e-5, 1e10].  -> (np.float32 mean, np.float32 std)."""
    n, s1, s2 = int(n), int(s1), int(s2)
    if n < 1:
        raise ValueError(f"tstream.delta_moments: n = {n}")
    mean = np.float32(s1 / n)
    var = (n * s2 - s1 * s1) / (n * (n - 1)) if n > 1 else 0.0
    std = np.float32(math.sqrt(var)) if var > 0 else np.float32(0.0)      # (a wrapped s2 can make the numerator negative: then 0, on both paths)
    return mean, np.float32(np.clip(std, np.float32(1e-5), np.float32(1e10)))


def eligible(count, lo, hi):
    """Whether a difference record on [lo, hi] of `count` symbols may be coded: -2^20 <= lo, hi <= 2^20, count <= 2^24."""
    return -MAX_DELTA <= int(lo) and int(hi) <= MAX_DELTA and int(count) <= MAX_COUNT
