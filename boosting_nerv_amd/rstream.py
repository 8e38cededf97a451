"""Container of a compressed video whose symbols decode on the device: the records of a version-1 CEM file
(bitstream.py) with every record's symbols cut into runs that are range-ANS coded independently, so that one kernel (csrc/rans.hip) decodes
the runs side by side.

Host-only code (numpy and struct), little-endian throughout; framing, cursor, settings header, embedding header and raw section are
container.py's.  This module is also the home of the run-coded CEM family's payload: estream.py, wstream.py and
tstream.py write and parse theirs through payload() and parse() with a Kind of their own:

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
import struct
from collections import namedtuple

import numpy as np

from . import container
from .container import F32 as _F32, U32 as _U32

MAGIC = b"BNRC"
VERSION = 1
_PREFIX = container.PREFIX            # (the name the tests of the kinds frame their damaged payloads with)
MIN_RUN, MAX_RUN, MAX_ALPHABET = 64, 4096, 4096      # BNERV_RANS_MIN_RUN, BNERV_RANS_MAX_RUN, BNERV_RANS_MAX_ALPHABET
PAD_WORDS = 2                                         # zero words after the last run
_RECORD = struct.Struct("<Ifffii")        # count, scale, mean, std, lo, hi
ITEMS = ("ans_words", "run_index", "tensor_side", "embed_side", "raw", "header", "padding")

RRecord = namedtuple("RRecord", "count scale mean std lo hi run_words beta", defaults=(None,))
RRecord.__doc__ = """One coded tensor.  scale / mean / std / beta: np.float32 (beta: None for a weight or bias);  run_words: uint16 array."""
RStream = namedtuple("RStream", "settings tensors embeds embed_shape raw words")
RStream.__doc__ = """settings: dict (with "ans_run");  tensors / embeds: [RRecord];  embed_shape: (C, h, w) or None;  raw: [float32 array];
words: uint32 array, every run of every record (tensors, then embeds) back to back, without the two padding words"""
Kind = namedtuple("Kind", "who magic items record pack_head read_head check_settings lead")
Kind.__doc__ = """What one kind of the family adds to the shared payload.  who: the name in its messages;  magic;  items: its budget items;  record: its
namedtuple, whose fields end with run_words and beta;  pack_head(r) -> bytes and read_head(cur, side) -> tuple: a record's fields in front of
run_words, count first;  check_settings(who, settings) -> the run length;  lead: whether a byte (booked as "embed_side") precedes every
embedding record (tstream.py: pred)."""


def check_run(run):
    if not isinstance(run, (int, np.integer)) or isinstance(run, bool) or not MIN_RUN <= run <= MAX_RUN or run % 64:
        raise ValueError(f"rstream: the run length is {run!r} (a multiple of 64 in {MIN_RUN}..{MAX_RUN})")
    return int(run)


def n_runs(count, run):
    return (int(count) + run - 1) // run


def check_range(who, count, lo, hi, limit=True):
    """A read record's count and symbol range; limit: whether the range must fit the table the device decoder holds."""
    if count == 0 or hi < lo:
        raise ValueError(f"{who}: a record of {count} symbols on the range [{lo}, {hi}]")
    if limit and hi - lo + 1 > MAX_ALPHABET:
        raise ValueError(f"{who}: a record's alphabet [{lo}, {hi}] has {hi - lo + 1} symbols; the device decoder holds {MAX_ALPHABET}")


def record_bytes(kind, r, with_beta):
    """A record as the file holds it: the kind's head, the words of every run, beta behind an embedding record."""
    return kind.pack_head(r) + np.ascontiguousarray(r.run_words, dtype="<u2").tobytes() + (_F32.pack(np.float32(r.beta)) if with_beta else b"")


def payload(kind, settings, tensors, embeds, embed_shape, raw, words, leads=()):
    """The payload of a file of `kind`.  leads: the byte in front of every embedding record, for a kind that has one."""
    run = kind.check_settings(kind.who + ".write", settings)
    for r in list(tensors) + list(embeds):
        if len(r.run_words) != n_runs(r.count, run):
            raise ValueError(f"{kind.who}.write: a record of {r.count} symbols with {len(r.run_words)} run lengths (runs of {run})")
    out = [container.header_bytes(settings), _U32.pack(len(tensors))] + [record_bytes(kind, r, False) for r in tensors]
    out.append(container.embed_head_bytes(kind.who, embeds, embed_shape))
    for k, r in enumerate(embeds):
        out.append((bytes([leads[k]]) if kind.lead else b"") + record_bytes(kind, r, True))
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    out += [container.raw_bytes(raw), _U32.pack(w.size + PAD_WORDS), w.tobytes(), b"\0" * (4 * PAD_WORDS)]
    return b"".join(out)


def _read_record(cur, kind, run, with_beta, side):
    head = kind.read_head(cur, side)
    run_words = cur.array("<u2", n_runs(head[0], run), "run_index")
    if int(run_words.min()) < 2:
        raise ValueError(f"{cur.who}: run {int(run_words.argmin())} of a record has {int(run_words.min())} words: fewer than its two state words")
    return kind.record(*head, run_words, cur.array("<f4", 1, side)[0] if with_beta else None)


def parse(kind, path_or_buffer):
    """-> ((settings, tensors, embeds, embed_shape, raw, words), budget, file size, leads) of a file of `kind`."""
    blob = container.blob_of(path_or_buffer)
    cur = container.Cursor(container.unframe(blob, kind.magic, VERSION, kind.who), kind.who, kind.items)
    settings = container.read_settings(cur)
    run = kind.check_settings(kind.who, settings)
    n_tensors, = cur.unpack(_U32, "header")
    tensors = [_read_record(cur, kind, run, False, "tensor_side") for _ in range(n_tensors)]
    n_embeds, embed_shape = container.read_embed_head(cur)
    embeds, leads = [], []
    for _ in range(n_embeds):
        if kind.lead:
            leads.append(cur.take(1, "embed_side")[0])
        embeds.append(_read_record(cur, kind, run, True, "embed_side"))
    raw = container.read_raw(cur)
    n_words, = cur.unpack(_U32, "header")
    words = cur.array("<u4", n_words, "ans_words")
    cur.end("the words")
    total = sum(int(r.run_words.sum(dtype=np.uint64)) for r in tensors + embeds)
    if total + PAD_WORDS != n_words:
        raise ValueError(f"{kind.who}: the run lengths of the records add up to {total} words, the payload has {n_words} (two of them padding)")
    if words[total:].any():
        raise ValueError(f"{kind.who}: the two words after the last run are not zero")
    cur.bits["ans_words"] -= 32 * PAD_WORDS
    cur.bits["padding"] = 32 * PAD_WORDS
    return (settings, tensors, embeds, embed_shape, raw, words[:total]), container.budget(cur, len(blob)), len(blob), leads


def _check_settings(who, settings):
    return check_run(settings.get("ans_run") if isinstance(settings, dict) else None)


def _pack_head(r):
    return _RECORD.pack(int(r.count), np.float32(r.scale), np.float32(r.mean), np.float32(r.std), int(r.lo), int(r.hi))


def _read_head(cur, side):
    count, scale, mean, std, lo, hi = cur.unpack(_RECORD, side)
    check_range(cur.who, count, lo, hi)
    return count, np.float32(scale), np.float32(mean), np.float32(std), lo, hi


KIND = Kind("rstream", MAGIC, ITEMS, RRecord, _pack_head, _read_head, _check_settings, False)


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    return container.frame(MAGIC, VERSION, payload(KIND, settings, list(tensors), list(embeds), embed_shape, list(raw), words))


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, tensors, embeds, embed_shape, raw, words))


def _parse(path_or_buffer):
    fields, bits, nbytes, _ = parse(KIND, path_or_buffer)
    return RStream(*fields), bits, nbytes


def read(path_or_buffer):
    """-> RStream(settings, tensors, embeds, embed_shape, raw, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits: "ans_words" (the words of all runs, their two state words each included), "run_index" (16 per
    run), "tensor_side" and "embed_side" (count, scale, mean, std, lo, hi of every record; + beta for an embedding), "raw" (the fp32
    section), "header" (the JSON settings, the section counts and the container's framing: magic, version, length, CRC) and "padding" (the
    two zero words) -- plus "total" = their sum = 8 * file size, "ans_run", and the counts "n_tensors", "n_embeds", "n_raw", "n_runs",
    "n_symbols", "bytes"."""
    rs, out, nbytes = _parse(path_or_buffer)
    recs = rs.tensors + rs.embeds
    out.update(total=8 * nbytes, ans_run=int(rs.settings["ans_run"]), n_tensors=len(rs.tensors), n_embeds=len(rs.embeds), n_raw=len(rs.raw),
               n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), bytes=nbytes)
    return out


def record_words(rs):
    """The word span of every record of a stream of the family, tensors then embeds: [(first word, word count)]."""
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
