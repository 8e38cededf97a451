"""Container of a compressed video whose records choose their symbol table: the chunked CEM file of rstream.py --
every record cut into runs that are range-ANS coded independently and decoded by one kernel (csrc/rans.hip) -- in which a record is coded
either under the Gaussian of its (mean, std), as there, or under a table of its own symbol frequencies that the file carries, whichever
makes the file smaller.

Host-only code (numpy and struct), little-endian throughout; the framing is rstream.py's:

    magic "BNRE" | version u32 (1) | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings of an rstream header, plus "ans_tables": "empirical" -- settings only)
                n_tensors u32 | n_tensors x record
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (record, beta f32)
                n_raw u32 | n_raw x (count u32 | count x f32)
                n_words u32 | n_words x u32                         (all runs of all records back to back, then two zero words)
    record  :=  count u32 | scale f32 | lo i32 | hi i32 | model u8
                | model 0: mean f32 | std f32
                | model 1: A = hi - lo + 1 values LEB128(f[k] - 1); every f[k] >= 1, their sum 2^24
                | ceil(count / ans_run) x u16 (words of every run)

Symbol lo + k of a model-1 record owns f[k] of the 2^24 slots: its cumulative table is the running sum.  Everything else -- record order,
raw section, runs, the two state words of a run -- is rstream.py's.

read() raises ValueError wherever rstream.read does, and for a header without "ans_tables": "empirical", a model byte other than 0 or 1, a
LEB128 value that runs past the payload, exceeds 2^24 or is padded with an empty last byte (one content, one file), and frequencies that
do not sum to 2^24.  info() books every bit of the file under one of eight items."""
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

from .bitstream import _blob
from .rstream import MAX_ALPHABET, PAD_WORDS, _F32, _PREFIX, _U32, check_run, n_runs

MAGIC = b"BNRE"
VERSION = 1
TOTAL = 1 << 24                            # slots of a table (the coder's 24-bit probabilities)
GAUSSIAN, TABLE = 0, 1                     # the model byte
_HEAD = struct.Struct("<IfiiB")            # count, scale, lo, hi, model
_MOMENTS = struct.Struct("<ff")            # mean, std
ITEMS = ("ans_words", "run_index", "tensor_side", "embed_side", "tables", "raw", "header", "padding")

ERecord = namedtuple("ERecord", "count scale lo hi model mean std freq run_words beta", defaults=(None,))
ERecord.__doc__ = """One coded tensor.  model GAUSSIAN: mean / std np.float32, freq None;  model TABLE: mean / std None, freq the uint32 slot count of
every symbol of [lo, hi].  scale / beta: np.float32 (beta: None for a weight or bias);  run_words: uint16 array."""
EStream = namedtuple("EStream", "settings tensors embeds embed_shape raw words")
EStream.__doc__ = """settings: dict (with "ans_run" and "ans_tables");  tensors / embeds: [ERecord];  embed_shape: (C, h, w) or None;  raw: [float32
array];  words: uint32 array, every run of every record (tensors, then embeds) back to back, without the two padding words"""


def leb128(values):
    """The unsigned LEB128 bytes of non-negative integers, one after the other."""
    out = bytearray()
    for v in values:
        v = int(v)
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
    return bytes(out)


def table_bytes(freq):
    """A model-1 record's table as the file stores it."""
    return leb128(np.asarray(freq, dtype=np.int64) - 1)


def _pack_record(out, r, with_beta):
    out.append(_HEAD.pack(int(r.count), np.float32(r.scale), int(r.lo), int(r.hi), int(r.model)))
    if r.model == GAUSSIAN:
        out.append(_MOMENTS.pack(np.float32(r.mean), np.float32(r.std)))
    elif r.model == TABLE:
        f = np.asarray(r.freq, dtype=np.int64).reshape(-1)
        if f.size != r.hi - r.lo + 1 or int(f.min()) < 1 or int(f.sum()) != TOTAL:
            raise ValueError(f"estream.write: a table of {f.size} frequencies (sum {int(f.sum())}, smallest {int(f.min())}) on the range [{r.lo}, {r.hi}]")
        out.append(table_bytes(f))
    else:
        raise ValueError(f"estream.write: model {r.model!r} (0: Gaussian, 1: table)")
    out.append(np.ascontiguousarray(r.run_words, dtype="<u2").tobytes())
    if with_beta:
        out.append(_F32.pack(np.float32(r.beta)))


def _payload(settings, tensors, embeds, embed_shape, raw, words):
    run = check_run(settings.get("ans_run"))
    if settings.get("ans_tables") != "empirical":
        raise ValueError('estream.write: the settings need "ans_tables": "empirical"')
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    out = [_U32.pack(len(header)), header, _U32.pack(len(tensors))]
    for r in list(tensors) + list(embeds):
        if len(r.run_words) != n_runs(r.count, run):
            raise ValueError(f"estream.write: a record of {r.count} symbols with {len(r.run_words)} run lengths (runs of {run})")
    for r in tensors:
        _pack_record(out, r, False)
    if embeds and embed_shape is None:
        raise ValueError("estream.write: embedding records need embed_shape (C, h, w)")
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
            raise ValueError(f"estream: truncated ({item} needs {n} bytes at offset {self.pos} of a {len(self.data)}-byte payload)")
        piece = self.data[self.pos:self.pos + n]
        self.pos += n
        self.bits[item] += 8 * n
        return piece

    def unpack(self, st, item):
        return st.unpack(self.take(st.size, item))

    def leb128(self, item):
        v, shift = 0, 0
        while True:
            if self.pos >= len(self.data):
                raise ValueError(f"estream: truncated (a LEB128 value of {item} runs past the {len(self.data)}-byte payload)")
            b = self.data[self.pos]
            self.pos += 1
            self.bits[item] += 8
            v |= (b & 0x7F) << shift
            shift += 7
            if v > TOTAL or shift > 28:                    # (shift: a value padded with continuation bytes)
                raise ValueError(f"estream: a LEB128 value of {item} exceeds 2^24")
            if not b & 0x80:
                if b == 0 and shift > 7:                   # one value, one spelling: the writer never ends on an empty group
                    raise ValueError(f"estream: a LEB128 value of {item} is padded with an empty last byte")
                return v


def _read_record(cur, run, with_beta, side):
    count, scale, lo, hi, model = cur.unpack(_HEAD, side)
    if count == 0 or hi < lo:
        raise ValueError(f"estream: a record of {count} symbols on the range [{lo}, {hi}]")
    if hi - lo + 1 > MAX_ALPHABET:
        raise ValueError(f"estream: a record's alphabet [{lo}, {hi}] has {hi - lo + 1} symbols; the device decoder holds {MAX_ALPHABET}")
    mean = std = freq = None
    if model == GAUSSIAN:
        mean, std = (np.float32(v) for v in cur.unpack(_MOMENTS, side))
    elif model == TABLE:
        freq = np.fromiter((cur.leb128("tables") + 1 for _ in range(hi - lo + 1)), dtype=np.int64, count=hi - lo + 1)
        if int(freq.sum()) != TOTAL:
            raise ValueError(f"estream: the frequencies of a record's table sum to {int(freq.sum())}, not 2^24")
        freq = freq.astype(np.uint32)
    else:
        raise ValueError(f"estream: a record's model byte is {model} (0: Gaussian, 1: table)")
    run_words = np.frombuffer(cur.take(2 * n_runs(count, run), "run_index"), dtype="<u2").astype(np.uint16)
    if int(run_words.min()) < 2:
        raise ValueError(f"estream: run {int(run_words.argmin())} of a record has {int(run_words.min())} words: fewer than its two state words")
    beta = np.frombuffer(cur.take(4, side), dtype="<f4")[0] if with_beta else None
    return ERecord(count, np.float32(scale), lo, hi, model, mean, std, freq, run_words, beta)


def _parse(path_or_buffer):
    blob = _blob(path_or_buffer)
    if len(blob) < _PREFIX.size:
        raise ValueError(f"estream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != MAGIC:
        raise ValueError(f"estream: bad magic number {magic!r} (want {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"estream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"estream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("estream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    n_header, = cur.unpack(_U32, "header")
    try:
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"estream: the settings header is not JSON ({e})") from None
    run = check_run(settings.get("ans_run") if isinstance(settings, dict) else None)
    if settings.get("ans_tables") != "empirical":
        raise ValueError(f'estream: the header\'s "ans_tables" is {settings.get("ans_tables")!r} (this kind says "empirical")')
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
        raise ValueError(f"estream: {len(payload) - cur.pos} payload bytes follow the words")
    total = sum(int(r.run_words.sum(dtype=np.uint64)) for r in tensors + embeds)
    if total + PAD_WORDS != n_words:
        raise ValueError(f"estream: the run lengths of the records add up to {total} words, the payload has {n_words} (two of them padding)")
    if words[total:].any():
        raise ValueError("estream: the two words after the last run are not zero")
    cur.bits["ans_words"] -= 32 * PAD_WORDS
    cur.bits["padding"] = 32 * PAD_WORDS
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return EStream(settings, tensors, embeds, (C_, h_, w_) if n_embeds else None, raw, words[:total]), cur.bits, len(blob)


def read(path_or_buffer):
    """-> EStream(settings, tensors, embeds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits: "ans_words" (the words of all runs, their two state words each included), "run_index" (16 per
    run), "tensor_side" and "embed_side" (count, scale, lo, hi and the model byte of every record; + mean, std under a Gaussian; + beta for
    an embedding), "tables" (the LEB128 frequencies of the records that carry a table), "raw" (the fp32 section), "header" (the JSON
    settings, the section counts and the container's framing) and "padding" (the two zero words) -- plus "total" = their sum = 8 * file
    size, "ans_run", and the counts "n_tensors", "n_embeds", "n_raw", "n_runs", "n_symbols", "n_table_records", "n_gaussian_records",
    "bytes"."""
    es, bits, nbytes = _parse(path_or_buffer)
    out = {k: int(bits[k]) for k in ITEMS}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    recs = es.tensors + es.embeds
    n_table = sum(r.model == TABLE for r in recs)
    out.update(total=total, ans_run=int(es.settings["ans_run"]), n_tensors=len(es.tensors), n_embeds=len(es.embeds), n_raw=len(es.raw),
               n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), n_table_records=int(n_table),
               n_gaussian_records=len(recs) - int(n_table), bytes=nbytes)
    return out


def record_words(es):
    """The word span of every record of an EStream, tensors then embeds: [(first word, word count)]."""
    spans, at = [], 0
    for r in es.tensors + es.embeds:
        n = int(r.run_words.sum(dtype=np.uint64))
        spans.append((at, n))
        at += n
    return spans


def record_cdf(r):
    """The cumulative table a record is coded under (uint32, hi - lo + 2 entries): the quantised Gaussian of the coder (csrc/ans.cpp) or the
    running sum of the record's own frequencies."""
    if r.model == TABLE:
        return np.concatenate([[0], np.cumsum(r.freq, dtype=np.uint64)]).astype(np.uint32)
    from .lib.entropy_model import ans_gaussian_cdf
    return ans_gaussian_cdf(r.lo, r.hi, float(r.mean), float(r.std))


def decode_record(es, k):
    """The symbols of record k (tensors, then embeds) of an EStream, decoded on the host (int32 numpy)."""
    from .lib.entropy_model import ans_decode_table_runs
    r = (es.tensors + es.embeds)[k]
    at, n = record_words(es)[k]
    return ans_decode_table_runs(es.words[at:at + n], r.run_words, r.count, r.lo, record_cdf(r), int(es.settings["ans_run"]))
