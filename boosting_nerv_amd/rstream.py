"""Container of a compressed video whose symbols decode on the device: the records of a version-1 CEM file
(bitstream.py) with every record's symbols cut into runs that are range-ANS coded independently, so that one kernel (csrc/rans.hip) decodes
the runs side by side.

Host-only code (numpy and struct), little-endian throughout; the framing is bitstream.py's:

    magic "BNRC" | version u32 (1) | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings of a version-1 CEM header, plus "ans_run" -- settings only, no code)
                n_tensors u32 | n_tensors x record                  (order of model._quant_modules(), weight before bias)
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (record, beta f32)      (HNeRV_Boost: one per frame; else all four 0)
                n_raw u32 | n_raw x (count u32 | count x f32)       (the decoder's state_dict entries no record covers, in its order)
                n_words u32 | n_words x u32                         (all runs of all records back to back, then two zero words)
    record  :=  count u32 | scale f32 | mean f32 | std f32 | lo i32 | hi i32 | ceil(count / ans_run) x u16 (words of every run)

The record order, the raw section and every (scale, mean, std, lo, hi, beta) are those of the version-1 file of the same evaluation; only
the coding of the symbols differs.  A run is a message of the coder of csrc/ans.cpp under its record's table, coded from an empty state:
its bulk words in refill order, then its final state as exactly two words (low, high).  A run never spans two records; the last run of a
record may be shorter.

read() raises ValueError for a bad magic number, an unknown version, a truncated file or a CRC mismatch (as bitstream.read does), and for
run word counts that do not add up to the payload's words, a run shorter than its two state words, an alphabet above 4096 symbols (the
kernel holds a record's table in LDS) and an ans_run that is not a multiple of 64 in 64..4096.  info() books every bit of the file under
one of seven items."""
import io
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

from .bitstream import _blob

MAGIC = b"BNRC"
VERSION = 1
MIN_RUN, MAX_RUN, MAX_ALPHABET = 64, 4096, 4096      # BNERV_RANS_MIN_RUN, BNERV_RANS_MAX_RUN, BNERV_RANS_MAX_ALPHABET
PAD_WORDS = 2                                         # zero words after the last run
_PREFIX = struct.Struct("<4sIQ")          # magic, version, payload length
_RECORD = struct.Struct("<Ifffii")        # count, scale, mean, std, lo, hi
_U32 = struct.Struct("<I")
_F32 = struct.Struct("<f")
ITEMS = ("ans_words", "run_index", "tensor_side", "embed_side", "raw", "header", "padding")

RRecord = namedtuple("RRecord", "count scale mean std lo hi run_words beta", defaults=(None,))
RRecord.__doc__ = """One coded tensor.  scale / mean / std / beta: np.float32 (beta: None for a weight or bias);  run_words: uint16 array."""
RStream = namedtuple("RStream", "settings tensors embeds embed_shape raw words")
RStream.__doc__ = """settings: dict (with "ans_run");  tensors / embeds: [RRecord];  embed_shape: (C, h, w) or None;  raw: [float32 array];
words: uint32 array, every run of every record (tensors, then embeds) back to back, without the two padding words"""


def check_run(run):
    if not isinstance(run, (int, np.integer)) or isinstance(run, bool) or not MIN_RUN <= run <= MAX_RUN or run % 64:
        raise ValueError(f"rstream: the run length is {run!r} (a multiple of 64 in {MIN_RUN}..{MAX_RUN})")
    return int(run)


def n_runs(count, run):
    return (int(count) + run - 1) // run


def _pack_record(out, r, with_beta):
    out.append(_RECORD.pack(int(r.count), np.float32(r.scale), np.float32(r.mean), np.float32(r.std), int(r.lo), int(r.hi)))
    out.append(np.ascontiguousarray(r.run_words, dtype="<u2").tobytes())
    if with_beta:
        out.append(_F32.pack(np.float32(r.beta)))


def _payload(settings, tensors, embeds, embed_shape, raw, words):
    run = check_run(settings.get("ans_run"))
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    out = [_U32.pack(len(header)), header, _U32.pack(len(tensors))]
    for r in list(tensors) + list(embeds):
        if len(r.run_words) != n_runs(r.count, run):
            raise ValueError(f"rstream.write: a record of {r.count} symbols with {len(r.run_words)} run lengths (runs of {run})")
    for r in tensors:
        _pack_record(out, r, False)
    if embeds and embed_shape is None:
        raise ValueError("rstream.write: embedding records need embed_shape (C, h, w)")
    out.append(struct.pack("<IIII", len(embeds), *(embed_shape if embeds else (0, 0, 0))))
    for r in embeds:
        _pack_record(out, r, True)
    out.append(_U32.pack(len(raw)))
    for a in raw:
        a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
        out.append(_U32.pack(a.size))
        out.append(a.tobytes())
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    out += [_U32.pack(w.size + PAD_WORDS), w.tobytes(), b"\0" * (4 * PAD_WORDS)]
    return b"".join(out)


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    payload = _payload(settings, list(tensors), list(embeds), embed_shape, list(raw), words)
    return _PREFIX.pack(MAGIC, VERSION, len(payload)) + payload + _U32.pack(zlib.crc32(payload) & 0xFFFFFFFF)


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    blob = to_bytes(settings, tensors, embeds, embed_shape, raw, words)
    if hasattr(path_or_buffer, "write"):
        path_or_buffer.write(blob)
    else:
        with open(path_or_buffer, "wb") as f:
            f.write(blob)
    return len(blob)


class _Cursor:
    """Bounds-checked reads of the payload; `bits` books every byte it hands out under the name of a budget item."""

    def __init__(self, data):
        self.data, self.pos, self.bits = data, 0, dict.fromkeys(ITEMS, 0)

    def take(self, n, item):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError(f"rstream: truncated ({item} needs {n} bytes at offset {self.pos} of a {len(self.data)}-byte payload)")
        piece = self.data[self.pos:self.pos + n]
        self.pos += n
        self.bits[item] += 8 * n
        return piece

    def unpack(self, st, item):
        return st.unpack(self.take(st.size, item))


def _read_record(cur, run, with_beta, side):
    count, scale, mean, std, lo, hi = cur.unpack(_RECORD, side)
    if count == 0 or hi < lo:
        raise ValueError(f"rstream: a record of {count} symbols on the range [{lo}, {hi}]")
    if hi - lo + 1 > MAX_ALPHABET:
        raise ValueError(f"rstream: a record's alphabet [{lo}, {hi}] has {hi - lo + 1} symbols; the device decoder holds {MAX_ALPHABET}")
    run_words = np.frombuffer(cur.take(2 * n_runs(count, run), "run_index"), dtype="<u2").astype(np.uint16)
    if int(run_words.min()) < 2:
        raise ValueError(f"rstream: run {int(run_words.argmin())} of a record has {int(run_words.min())} words: fewer than its two state words")
    beta = np.frombuffer(cur.take(4, side), dtype="<f4")[0] if with_beta else None
    return RRecord(count, np.float32(scale), np.float32(mean), np.float32(std), lo, hi, run_words, beta)


def _parse(path_or_buffer):
    blob = _blob(path_or_buffer)
    if len(blob) < _PREFIX.size:
        raise ValueError(f"rstream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != MAGIC:
        raise ValueError(f"rstream: bad magic number {magic!r} (want {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"rstream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"rstream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("rstream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    n_header, = cur.unpack(_U32, "header")
    try:
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"rstream: the settings header is not JSON ({e})") from None
    run = check_run(settings.get("ans_run") if isinstance(settings, dict) else None)
    n_tensors, = cur.unpack(_U32, "header")
    tensors = [_read_record(cur, run, False, "tensor_side") for _ in range(n_tensors)]
    n_embeds, C_, h_, w_ = cur.unpack(struct.Struct("<IIII"), "header")
    embeds = [_read_record(cur, run, True, "embed_side") for _ in range(n_embeds)]
    n_raw, = cur.unpack(_U32, "header")
    raw = []
    for _ in range(n_raw):
        cnt, = cur.unpack(_U32, "raw")
        raw.append(np.frombuffer(cur.take(4 * cnt, "raw"), dtype="<f4").astype(np.float32))
    n_words, = cur.unpack(_U32, "header")
    words = np.frombuffer(cur.take(4 * n_words, "ans_words"), dtype="<u4").astype(np.uint32)
    if cur.pos != len(payload):
        raise ValueError(f"rstream: {len(payload) - cur.pos} payload bytes follow the words")
    total = sum(int(r.run_words.sum(dtype=np.uint64)) for r in tensors + embeds)
    if total + PAD_WORDS != n_words:
        raise ValueError(f"rstream: the run lengths of the records add up to {total} words, the payload has {n_words} (two of them padding)")
    if words[total:].any():
        raise ValueError("rstream: the two words after the last run are not zero")
    cur.bits["ans_words"] -= 32 * PAD_WORDS
    cur.bits["padding"] = 32 * PAD_WORDS
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return RStream(settings, tensors, embeds, (C_, h_, w_) if n_embeds else None, raw, words[:total]), cur.bits, len(blob)


def read(path_or_buffer):
    """-> RStream(settings, tensors, embeds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits: "ans_words" (the words of all runs, their two state words each included), "run_index" (16 per
    run), "tensor_side" and "embed_side" (count, scale, mean, std, lo, hi of every record; + beta for an embedding), "raw" (the fp32
    section), "header" (the JSON settings, the section counts and the container's framing: magic, version, length, CRC) and "padding" (the
    two zero words) -- plus "total" = their sum = 8 * file size, "ans_run", and the counts "n_tensors", "n_embeds", "n_raw", "n_runs",
    "n_symbols", "bytes"."""
    rs, bits, nbytes = _parse(path_or_buffer)
    out = {k: int(bits[k]) for k in ITEMS}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    recs = rs.tensors + rs.embeds
    out.update(total=total, ans_run=int(rs.settings["ans_run"]), n_tensors=len(rs.tensors), n_embeds=len(rs.embeds), n_raw=len(rs.raw),
               n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), bytes=nbytes)
    return out


def record_words(rs):
    """The word span of every record of an RStream, tensors then embeds: [(first word, word count)]."""
    spans, at = [], 0
    for r in rs.tensors + rs.embeds:
        n = int(r.run_words.sum(dtype=np.uint64))
        spans.append((at, n))
        at += n
    return spans


def decode_record(rs, k):
    """The symbols of record k (tensors, then embeds) of an RStream, decoded on the host (int32 numpy)."""
    from .lib.entropy_model import ans_decode_gaussian_runs
    r = (rs.tensors + rs.embeds)[k]
    at, n = record_words(rs)[k]
    return ans_decode_gaussian_runs(rs.words[at:at + n], r.run_words, r.count, r.lo, r.hi, float(r.mean), float(r.std), int(rs.settings["ans_run"]))
