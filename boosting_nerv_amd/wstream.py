"""Container of a compressed video whose records may span any number of symbol values: the chunked CEM file of
estream.py -- every record cut into runs that are range-ANS coded independently, under its Gaussian or a table the file carries, and decoded
by one kernel -- in which a record has a `shift` k: a symbol v is written as  v - lo = (bucket << k) | low,  the bucket under a table of
B = ceil((hi - lo + 1) / 2^k) <= 4096 entries, `low` as k raw bits in the same rANS state.  k is the smallest shift with B <= 4096, so a
record of at most 4096 values has k = 0 and the words estream.py gives it.

Host-only code (numpy and struct), little-endian throughout; the framing is container.py's, the payload around the records rstream.py's and the
Gaussian-or-table half of a record estream.py's:

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
import struct
from collections import namedtuple

import numpy as np

from . import container, rstream
from .estream import GAUSSIAN, ITEMS, TABLE, TOTAL, model_bytes, read_model, table_bytes      # noqa: F401  (re-exported)
from .rstream import MAX_ALPHABET, PAD_WORDS, check_run, n_runs, record_words      # noqa: F401  (re-exported)

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


def _pack_head(r):
    _check_shape("wstream.write", int(r.lo), int(r.hi), int(r.shift))
    return (_HEAD.pack(int(r.count), np.float32(r.scale), int(r.lo), int(r.hi), int(r.model), int(r.shift))
            + model_bytes("wstream", r, n_buckets(r.lo, r.hi, r.shift), f"[{r.lo}, {r.hi}] at shift {r.shift}"))


def _read_head(cur, side):
    count, scale, lo, hi, model, shift = cur.unpack(_HEAD, side)
    rstream.check_range(cur.who, count, lo, hi, limit=False)
    _check_shape(cur.who, lo, hi, shift)
    return (count, np.float32(scale), lo, hi, model, shift, *read_model(cur, side, model, n_buckets(lo, hi, shift)))


def _check_settings(who, settings):
    run = check_run(settings.get("ans_run") if isinstance(settings, dict) else None)
    if settings.get("ans_tables") not in TABLES:
        raise ValueError(f'{who}: the header\'s "ans_tables" is {settings.get("ans_tables")!r} ({" | ".join(TABLES)})')
    if settings.get("ans_wide") is not True:
        raise ValueError(f'{who}: the header\'s "ans_wide" is {settings.get("ans_wide")!r} (this kind says true)')
    return run


KIND = rstream.Kind("wstream", MAGIC, ITEMS, WRecord, _pack_head, _read_head, _check_settings, False)


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    return container.frame(MAGIC, VERSION, rstream.payload(KIND, settings, list(tensors), list(embeds), embed_shape, list(raw), words))


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, tensors, embeds, embed_shape, raw, words))


def _parse(path_or_buffer):
    fields, bits, nbytes, _ = rstream.parse(KIND, path_or_buffer)
    return WStream(*fields), bits, nbytes


def read(path_or_buffer):
    """-> WStream(settings, tensors, embeds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits, under estream.info's eight items (the shift byte of a record counts as its side) -- plus "total" =
    their sum = 8 * file size, "ans_run", "ans_tables" and estream.info's counts, "n_wide_records" (records with a shift above 0) and
    "max_shift"."""
    return _budget(*_parse(path_or_buffer))


def _budget(ws, out, nbytes):
    recs = ws.tensors + ws.embeds
    n_table = sum(r.model == TABLE for r in recs)
    out.update(total=8 * nbytes, ans_run=int(ws.settings["ans_run"]), ans_tables=ws.settings["ans_tables"], n_tensors=len(ws.tensors), n_embeds=len(ws.embeds),
               n_raw=len(ws.raw), n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), n_table_records=int(n_table),
               n_gaussian_records=len(recs) - int(n_table), n_wide_records=int(sum(r.shift > 0 for r in recs)),
               max_shift=int(max((r.shift for r in recs), default=0)), bytes=nbytes)
    return out


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
