"""Container of a compressed video whose records may span any number of symbol values: the chunked CEM file of
estream.py -- every record cut into runs that are range-ANS coded independently, under its Gaussian or a table the file carries, and decoded
by one kernel -- in which a record has a `shift` k: a symbol v is written as  v - lo = (bucket << k) | low,  the bucket under a table of
B = ceil((hi - lo + 1) / 2^k) <= 4096 entries, `low` as k raw bits in the same rANS state.  k is the smallest shift with B <= 4096, so a
record of at most 4096 values has k = 0 and the words estream.py gives it.

Host-only code (numpy and struct), little-endian throughout; framing and payload are estream.py's:

    magic "BNRW" | version u32 (1) | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings of an estream header -- "ans_tables": "gaussian" | "empirical" --
                plus "ans_wide": true)
                n_tensors u32 | n_tensors x record
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (record, beta f32)
                n_raw u32 | n_raw x (count u32 | count x f32)
                n_words u32 | n_words x u32                         (all runs of all records back to back, then two zero words)
    record  :=  count u32 | scale f32 | lo i32 | hi i32 | model u8 | shift u8
                | model 0: mean f32 | std f32
                | model 1: B values LEB128(f[j] - 1); every f[j] >= 1, their sum 2^24
                | ceil(count / ans_run) x u16 (words of every run)

Bucket j of a model-1 record owns f[j] of the 2^24 slots; a model-0 record's table is the quantised Gaussian over the bucket edges
(csrc/ans.cpp, bnerv_ans_gaussian_bucket_cdf).

read() raises ValueError wherever estream.read does (the 4096-value limit excepted), and for a header without "ans_wide": true, a shift
that is not the minimal one of [lo, hi] (one content, one spelling), a shift above 16 and a table of fewer than two buckets.  info() books
every bit of the file under estream's eight items; the shift byte counts as side."""
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

from .bitstream import _blob
from .estream import GAUSSIAN, ITEMS, TABLE, TOTAL, _Cursor, _MOMENTS, table_bytes
from .rstream import MAX_ALPHABET, PAD_WORDS, _F32, _PREFIX, _U32, check_run, n_runs

MAGIC = b"BNRW"
VERSION = 1
MAX_SHIFT = 16                             # BNERV_RANSW_MAX_SHIFT: spans up to 4096 * 2^16 = 2^28 values
TABLES = ("gaussian", "empirical")
_HEAD = struct.Struct("<IfiiBB")           # count, scale, lo, hi, model, shift

WRecord = namedtuple("WRecord", "count scale lo hi model shift mean std freq run_words beta", defaults=(None,))
WRecord.__doc__ = """One coded tensor.  shift: the low bits of a symbol that go raw;  model GAUSSIAN: mean / std np.float32, freq None;  model TABLE:
mean / std None, freq the uint32 slot count of every bucket.  scale / beta: np.float32 (beta: None for a weight or bias);  run_words: uint16 array."""
WStream = namedtuple("WStream", "settings tensors embeds embed_shape raw words")
WStream.__doc__ = """settings: dict (with "ans_run", "ans_tables" and "ans_wide");  tensors / embeds: [WRecord];  embed_shape: (C, h, w) or None;  raw:
[float32 array];  words: uint32 array, every run of every record (tensors, then embeds) back to back, without the two padding words"""


def min_shift(lo, hi):
    """The shift of a record on [lo, hi]: the smallest k >= 0 with ceil((hi - lo + 1) / 2^k) <= 4096."""
    k = 0
    while n_buckets(lo, hi, k) > MAX_ALPHABET:
        k += 1
    return k


def n_buckets(lo, hi, shift):
    return (int(hi) - int(lo) + (1 << shift)) >> shift


def slot_words(run, shift):
    """The bound on the words of a run of `run` symbols at `shift` (two state words included)."""
    return run * (24 + shift) // 32 + 3


def _check_shape(who, lo, hi, shift):
    if hi < lo:
        raise ValueError(f"{who}: a record on the range [{lo}, {hi}]")
    if not 0 <= shift <= MAX_SHIFT:
        raise ValueError(f"{who}: a record's shift is {shift} (0..{MAX_SHIFT})")
    if shift != min_shift(lo, hi):
        raise ValueError(f"{who}: a record on [{lo}, {hi}] has shift {shift}; the minimal one is {min_shift(lo, hi)} (one content has one spelling)")
    if n_buckets(lo, hi, shift) < 2:
        raise ValueError(f"{who}: a record on [{lo}, {hi}] has a table of {n_buckets(lo, hi, shift)} bucket (at least 2)")


def _pack_record(out, r, with_beta):
    _check_shape("wstream.write", int(r.lo), int(r.hi), int(r.shift))
    out.append(_HEAD.pack(int(r.count), np.float32(r.scale), int(r.lo), int(r.hi), int(r.model), int(r.shift)))
    if r.model == GAUSSIAN:
        out.append(_MOMENTS.pack(np.float32(r.mean), np.float32(r.std)))
    elif r.model == TABLE:
        f = np.asarray(r.freq, dtype=np.int64).reshape(-1)
        if f.size != n_buckets(r.lo, r.hi, r.shift) or int(f.min()) < 1 or int(f.sum()) != TOTAL:
            raise ValueError(f"wstream.write: a table of {f.size} frequencies (sum {int(f.sum())}, smallest {int(f.min())}) on the range [{r.lo}, {r.hi}] "
                             f"at shift {r.shift}")
        out.append(table_bytes(f))
    else:
        raise ValueError(f"wstream.write: model {r.model!r} (0: Gaussian, 1: table)")
    out.append(np.ascontiguousarray(r.run_words, dtype="<u2").tobytes())
    if with_beta:
        out.append(_F32.pack(np.float32(r.beta)))


def _check_settings(who, settings):
    run = check_run(settings.get("ans_run") if isinstance(settings, dict) else None)
    if settings.get("ans_tables") not in TABLES:
        raise ValueError(f'{who}: the header\'s "ans_tables" is {settings.get("ans_tables")!r} ({" | ".join(TABLES)})')
    if settings.get("ans_wide") is not True:
        raise ValueError(f'{who}: the header\'s "ans_wide" is {settings.get("ans_wide")!r} (this kind says true)')
    return run


def _payload(settings, tensors, embeds, embed_shape, raw, words, check_settings=_check_settings, lead=None):
    """lead: None, or one bytes object per embedding record, written in front of it (tstream.py: the pred byte)."""
    run = check_settings("wstream.write", settings)
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    out = [_U32.pack(len(header)), header, _U32.pack(len(tensors))]
    for r in list(tensors) + list(embeds):
        if len(r.run_words) != n_runs(r.count, run):
            raise ValueError(f"wstream.write: a record of {r.count} symbols with {len(r.run_words)} run lengths (runs of {run})")
    for r in tensors:
        _pack_record(out, r, False)
    if embeds and embed_shape is None:
        raise ValueError("wstream.write: embedding records need embed_shape (C, h, w)")
    out.append(struct.pack("<IIII", len(embeds), *(embed_shape if embeds else (0, 0, 0))))
    for k, r in enumerate(embeds):
        if lead is not None:
            out.append(lead[k])
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


def _read_record(cur, run, with_beta, side):
    count, scale, lo, hi, model, shift = cur.unpack(_HEAD, side)
    if count == 0 or hi < lo:
        raise ValueError(f"wstream: a record of {count} symbols on the range [{lo}, {hi}]")
    _check_shape("wstream", lo, hi, shift)
    B = n_buckets(lo, hi, shift)
    mean = std = freq = None
    if model == GAUSSIAN:
        mean, std = (np.float32(v) for v in cur.unpack(_MOMENTS, side))
    elif model == TABLE:
        freq = np.fromiter((cur.leb128("tables") + 1 for _ in range(B)), dtype=np.int64, count=B)
        if int(freq.sum()) != TOTAL:
            raise ValueError(f"wstream: the frequencies of a record's table sum to {int(freq.sum())}, not 2^24")
        freq = freq.astype(np.uint32)
    else:
        raise ValueError(f"wstream: a record's model byte is {model} (0: Gaussian, 1: table)")
    run_words = np.frombuffer(cur.take(2 * n_runs(count, run), "run_index"), dtype="<u2").astype(np.uint16)
    if int(run_words.min()) < 2:
        raise ValueError(f"wstream: run {int(run_words.argmin())} of a record has {int(run_words.min())} words: fewer than its two state words")
    beta = np.frombuffer(cur.take(4, side), dtype="<f4")[0] if with_beta else None
    return WRecord(count, np.float32(scale), lo, hi, model, shift, mean, std, freq, run_words, beta)


def _parse(path_or_buffer, magic_want=MAGIC, who="wstream", check_settings=_check_settings, lead=None):
    """-> (WStream, bits, file size, leads).  The hooks are tstream.py's, whose file is this one with another magic, a settings check of its own and
    a byte in front of every embedding record: lead(cur, k) reads what precedes embedding record k; leads: what it returned."""
    try:
        return _parse_file(_blob(path_or_buffer), magic_want, check_settings, lead)
    except ValueError as e:
        if who == "wstream":
            raise
        raise ValueError(str(e).replace("wstream:", who + ":", 1)) from None


def _parse_file(blob, magic_want, check_settings, lead):
    if len(blob) < _PREFIX.size:
        raise ValueError(f"wstream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != magic_want:
        raise ValueError(f"wstream: bad magic number {magic!r} (want {magic_want!r})")
    if version != VERSION:
        raise ValueError(f"wstream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"wstream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("wstream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    try:
        return _parse_payload(cur, payload, len(blob), check_settings, lead)
    except ValueError as e:                                # (the cursor is estream's and says so)
        raise ValueError(str(e).replace("estream:", "wstream:", 1)) from None


def _parse_payload(cur, payload, nbytes, check_settings, lead):
    n_header, = cur.unpack(_U32, "header")
    try:
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"wstream: the settings header is not JSON ({e})") from None
    run = check_settings("wstream", settings)
    n_tensors, = cur.unpack(_U32, "header")
    tensors = [_read_record(cur, run, False, "tensor_side") for _ in range(n_tensors)]
    n_embeds, C_, h_, w_ = cur.unpack(struct.Struct("<IIII"), "header")
    embeds, leads = [], []
    for k in range(n_embeds):
        if lead is not None:
            leads.append(lead(cur, k))
        embeds.append(_read_record(cur, run, True, "embed_side"))
    n_raw, = cur.unpack(_U32, "header")
    raw = []
    for _ in range(n_raw):
        cnt, = cur.unpack(_U32, "raw")
        raw.append(np.frombuffer(cur.take(4 * cnt, "raw"), dtype="<f4").astype(np.float32))
    n_words, = cur.unpack(_U32, "header")
    words = np.frombuffer(cur.take(4 * n_words, "ans_words"), dtype="<u4").astype(np.uint32)
    if cur.pos != len(payload):
        raise ValueError(f"wstream: {len(payload) - cur.pos} payload bytes follow the words")
    total = sum(int(r.run_words.sum(dtype=np.uint64)) for r in tensors + embeds)
    if total + PAD_WORDS != n_words:
        raise ValueError(f"wstream: the run lengths of the records add up to {total} words, the payload has {n_words} (two of them padding)")
    if words[total:].any():
        raise ValueError("wstream: the two words after the last run are not zero")
    cur.bits["ans_words"] -= 32 * PAD_WORDS
    cur.bits["padding"] = 32 * PAD_WORDS
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return WStream(settings, tensors, embeds, (C_, h_, w_) if n_embeds else None, raw, words[:total]), cur.bits, nbytes, leads


def read(path_or_buffer):
    """-> WStream(settings, tensors, embeds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits, under estream.info's eight items (the shift byte of a record counts as its side) -- plus "total" =
    their sum = 8 * file size, "ans_run", "ans_tables" and estream.info's counts, "n_wide_records" (records with a shift above 0) and
    "max_shift"."""
    return _budget(*_parse(path_or_buffer)[:3])


def _budget(ws, bits, nbytes):
    out = {k: int(bits[k]) for k in ITEMS}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    recs = ws.tensors + ws.embeds
    n_table = sum(r.model == TABLE for r in recs)
    out.update(total=total, ans_run=int(ws.settings["ans_run"]), ans_tables=ws.settings["ans_tables"], n_tensors=len(ws.tensors), n_embeds=len(ws.embeds),
               n_raw=len(ws.raw), n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), n_table_records=int(n_table),
               n_gaussian_records=len(recs) - int(n_table), n_wide_records=int(sum(r.shift > 0 for r in recs)),
               max_shift=int(max((r.shift for r in recs), default=0)), bytes=nbytes)
    return out


def record_words(ws):
    """The word span of every record of a WStream, tensors then embeds: [(first word, word count)]."""
    spans, at = [], 0
    for r in ws.tensors + ws.embeds:
        n = int(r.run_words.sum(dtype=np.uint64))
        spans.append((at, n))
        at += n
    return spans


def record_cdf(r):
    """The cumulative table a record's buckets are coded under (uint32, B + 1 entries): the quantised Gaussian over the bucket edges
    (csrc/ans.cpp) or the running sum of the record's own frequencies."""
    if r.model == TABLE:
        return np.concatenate([[0], np.cumsum(r.freq, dtype=np.uint64)]).astype(np.uint32)
    from .lib.entropy_model import ans_gaussian_bucket_cdf
    return ans_gaussian_bucket_cdf(r.lo, r.hi, r.shift, float(r.mean), float(r.std))


def decode_record(ws, k):
    """The symbols of record k (tensors, then embeds) of a WStream, decoded on the host (int32 numpy)."""
    from .lib.entropy_model import ans_decode_wide_runs
    r = (ws.tensors + ws.embeds)[k]
    at, n = record_words(ws)[k]
    return ans_decode_wide_runs(ws.words[at:at + n], r.run_words, r.count, r.lo, r.hi, record_cdf(r), r.shift, int(ws.settings["ans_run"]))
