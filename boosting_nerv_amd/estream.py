"""Container of a compressed video whose records choose their symbol table: the chunked CEM file of rstream.py --
every record cut into runs that are range-ANS coded independently and decoded by one kernel (csrc/rans.hip) -- in which a record is coded
either under the Gaussian of its (mean, std), as there, or under a table of its own symbol frequencies that the file carries, whichever
makes the file smaller.

Host-only code (numpy and struct), little-endian throughout; the framing is container.py's and the payload around the records rstream.py's
(DESIGN section 40).  The Gaussian-or-table half of a record -- model_bytes(), read_model() -- is shared with wstream.py:

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
import struct
from collections import namedtuple

import numpy as np

from . import container, rstream
from .rstream import MAX_ALPHABET, PAD_WORDS, check_run, n_runs, record_words      # noqa: F401  (re-exported)

MAGIC = b"BNRE"
VERSION = 1
TOTAL = container.LEB128_MAX               # slots of a table (the coder's 24-bit probabilities)
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


def model_bytes(who, r, n, where):
    """What follows a record's model byte: mean and std, or the table of its n frequencies; where: the record's place, for the refusal."""
    if r.model == GAUSSIAN:
        return _MOMENTS.pack(np.float32(r.mean), np.float32(r.std))
    if r.model != TABLE:
        raise ValueError(f"{who}.write: model {r.model!r} (0: Gaussian, 1: table)")
    f = np.asarray(r.freq, dtype=np.int64).reshape(-1)
    if f.size != n or int(f.min()) < 1 or int(f.sum()) != TOTAL:
        raise ValueError(f"{who}.write: a table of {f.size} frequencies (sum {int(f.sum())}, smallest {int(f.min())}) on the range {where}")
    return table_bytes(f)


def read_model(cur, side, model, n):
    """What model_bytes wrote -> (mean, std, freq): two np.float32 and None, or None twice and the n uint32 frequencies."""
    if model == GAUSSIAN:
        return (*(np.float32(v) for v in cur.unpack(_MOMENTS, side)), None)
    if model != TABLE:
        raise ValueError(f"{cur.who}: a record's model byte is {model} (0: Gaussian, 1: table)")
    freq = np.fromiter((cur.leb128("tables") + 1 for _ in range(n)), dtype=np.int64, count=n)
    if int(freq.sum()) != TOTAL:
        raise ValueError(f"{cur.who}: the frequencies of a record's table sum to {int(freq.sum())}, not 2^24")
    return None, None, freq.astype(np.uint32)


def _pack_head(r):
    return (_HEAD.pack(int(r.count), np.float32(r.scale), int(r.lo), int(r.hi), int(r.model))
            + model_bytes("estream", r, r.hi - r.lo + 1, f"[{r.lo}, {r.hi}]"))


def _read_head(cur, side):
    count, scale, lo, hi, model = cur.unpack(_HEAD, side)
    rstream.check_range(cur.who, count, lo, hi)
    return (count, np.float32(scale), lo, hi, model, *read_model(cur, side, model, hi - lo + 1))


def _check_settings(who, settings):
    run = check_run(settings.get("ans_run") if isinstance(settings, dict) else None)
    if settings.get("ans_tables") != "empirical":
        raise ValueError(f'{who}: the header\'s "ans_tables" is {settings.get("ans_tables")!r} (this kind says "empirical")')
    return run


KIND = rstream.Kind("estream", MAGIC, ITEMS, ERecord, _pack_head, _read_head, _check_settings, False)


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    return container.frame(MAGIC, VERSION, rstream.payload(KIND, settings, list(tensors), list(embeds), embed_shape, list(raw), words))


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=(), words=()):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, tensors, embeds, embed_shape, raw, words))


def _parse(path_or_buffer):
    fields, bits, nbytes, _ = rstream.parse(KIND, path_or_buffer)
    return EStream(*fields), bits, nbytes


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
    es, out, nbytes = _parse(path_or_buffer)
    recs = es.tensors + es.embeds
    n_table = sum(r.model == TABLE for r in recs)
    out.update(total=8 * nbytes, ans_run=int(es.settings["ans_run"]), n_tensors=len(es.tensors), n_embeds=len(es.embeds), n_raw=len(es.raw),
               n_runs=int(sum(r.run_words.size for r in recs)), n_symbols=int(sum(r.count for r in recs)), n_table_records=int(n_table),
               n_gaussian_records=len(recs) - int(n_table), bytes=nbytes)
    return out


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
