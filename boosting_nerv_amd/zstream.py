"""Container of a SPARSE post-hoc quantised model: the twin of hnerv_utils.quant_tensor_sparse, in which a zero weight
stays exactly zero, under ONE Huffman code whose alphabet has leaves for zeros.  A sibling of qstream.py: the same
JSON header, record order and grid geometry, written and parsed by qstream.py's section functions; its own are the
leaves for zeros, `kept` and the header's zero-leaf count.

Host-only code (numpy and struct), little-endian throughout:

    magic "BNRZ" | version u32 | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings of a qstream header plus zero_parse "single" | "runs" and
                                            n_zero_leaves, the number of zero-run leaves in the bit string)
                266 x u8 code length              (leaves 0..255: the 8-bit codes; 256 + k, k = 0..8: 2^k consecutive zero elements;
                                                   265: the EOF leaf, never written; 0 = unused)
                n_records u32 | n_records x record
                n_words u32 | n_words x u32       (the bit string)
    record  :=  count u32 | outer u32 | red u32 | inner u32 | dtype u32 (0 fp32, 1 fp16) | kept u32 (the non-zero elements; dense: == count)
                outer * inner x min | outer * inner x scale
                ceil(count / huff_run) x u16      (bit length of every run)

Runs.  A record's ELEMENTS are cut into runs of huff_run = 256.  Inside a run a kept element is written as its code and every maximal
stretch of z zero elements -- clipped at the run's ends -- as z leaves 256 (parse "single") or as the leaves 256 + k of the set bits of z,
highest first (parse "runs": at most 9 leaves, z = 256 is one).  A run holds at most 256 leaves of at most 32 bits, so its length fits 16
bits.  The encoder writes the parse with fewer symbol bits ("single" on a tie); a decoder needs no case for it: it reads leaves until the
run's element count is reached.

read() raises ValueError on everything qstream.read refuses, on kept > count and on a header without a valid zero_parse / n_zero_leaves.
info() books every bit under the six items of qstream.info and adds n_zero_elements, n_zero_leaves and zero_parse."""
from collections import namedtuple

import numpy as np

from . import container, qstream
from .qstream import F16, F32, ITEMS, RUN, _header, magic_of, n_runs, stored_frames_item     # noqa: F401  (re-exported)

MAGIC = b"BNRZ"
VERSION = 1
_PREFIX = container.PREFIX            # (the name the tests of the kinds frame their damaged payloads with)
LEAVES = 266                              # BNERV_HUFFZ_LEAVES
ZERO = 256                                # BNERV_HUFFZ_ZERO: leaf ZERO + k is 2^k zero elements
ZERO_LEAVES = 9                           # BNERV_HUFFZ_ZERO_LEAVES
PARSES = ("single", "runs")               # BNERV_HUFFZ_SINGLE, BNERV_HUFFZ_RUNS, by index

ZRecord = namedtuple("ZRecord", "count outer red inner dtype kept min scale run_bits")
ZRecord.__doc__ = """One quantised tensor.  kept: its non-zero elements;  the rest as qstream.QRecord."""
ZStream = namedtuple("ZStream", "settings lengths records words")
ZStream.__doc__ = """settings: dict;  lengths: uint8 [266];  records: [ZRecord];  words: uint32 array (the bit string)"""


def check_lengths(lengths):
    """ValueError unless the 266 lengths describe a complete prefix code this format carries."""
    qstream.check_lengths(lengths, LEAVES, "zstream")


def _check_kept(who, count, outer, red, inner, dtype, kept):
    if kept > count:
        raise ValueError(f"{who}: a record of {count} elements announces {kept} kept ones")


SECTION = qstream.Section("zstream", LEAVES, ZRecord, _check_kept)


def parse_histogram(symbols, keep, counts, parse, run=RUN):
    """How often each of the 265 data leaves is written when the records (counts[k] elements each, back to back in `symbols` / `keep`) are
    parsed as `parse`: an int64 array of LEAVES - 1 bins.  A stretch of zeros ends at a kept element, at a run's end and at a record's end."""
    if parse not in PARSES:
        raise ValueError(f"zstream: parse = {parse!r} ({' | '.join(PARSES)})")
    if not 1 <= run <= RUN:
        raise ValueError(f"zstream: runs of {run} elements (1..{RUN}: a zero-run leaf covers at most {RUN})")
    sym = np.asarray(symbols).reshape(-1)
    kp = np.asarray(keep).reshape(-1) != 0
    n = sym.size
    if kp.size != n or int(np.sum(np.asarray(counts, dtype=np.int64))) != n:
        raise ValueError("zstream: symbols, keep and counts disagree on the number of elements")
    hist = np.zeros(LEAVES - 1, dtype=np.int64)
    hist[:256] = np.bincount(sym[kp], minlength=256)
    if parse == "single":
        hist[ZERO] = n - int(kp.sum())
        return hist
    first = np.zeros(n, dtype=bool)                       # the first element of every run
    at = 0
    for c in counts:
        first[at:at + int(c):run] = True
        at += int(c)
    zero = ~kp
    begins = zero & (first | np.concatenate([[True], kp[:-1]]))
    ends = zero & np.concatenate([first[1:] | kp[1:], [True]])
    z = np.flatnonzero(ends) - np.flatnonzero(begins) + 1
    for k in range(ZERO_LEAVES):
        hist[ZERO + k] = int(np.count_nonzero((z >> k) & 1))
    return hist


def _section(lengths, records, words):
    if np.size(lengths) != LEAVES:
        raise ValueError(f"zstream.write: the code table needs {LEAVES} lengths, got {np.size(lengths)}")
    return qstream.section_bytes(SECTION, lengths, records, words)


def to_bytes(settings, lengths, records, words):
    return container.frame(MAGIC, VERSION, b"".join(_header(settings) + _section(lengths, list(records), words)))


def write(path_or_buffer, settings, lengths, records, words):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, lengths, records, words))


def check_settings(who, settings):
    """What a header with a sparse tensor section must say -> its run length."""
    run = settings.get("huff_run")
    if not isinstance(run, int) or not 1 <= run <= RUN:
        raise ValueError(f"{who}: the header's run length is {run!r}")
    zero_leaves = settings.get("n_zero_leaves")
    if settings.get("zero_parse") not in PARSES or not isinstance(zero_leaves, int) or zero_leaves < 0:
        raise ValueError(f"{who}: the header's zero_parse / n_zero_leaves are {settings.get('zero_parse')!r} / {zero_leaves!r}")
    return run


def book_section(cur, settings, records, total, n_words):
    """qstream.book_section, and the header's zero-run leaves against the records -> the zero elements of the records."""
    zero_leaves, zeros = settings["n_zero_leaves"], sum(r.count - r.kept for r in records)
    qstream.book_section(cur, total, n_words)
    if zero_leaves > zeros or (zero_leaves == 0) != (zeros == 0) or (settings["zero_parse"] == "single" and zero_leaves != zeros):
        raise ValueError(f"{cur.who}: the header announces {zero_leaves} zero-run leaves ({settings['zero_parse']}), the records hold {zeros} zero elements")
    return zeros


def _parse(path_or_buffer):
    blob = container.blob_of(path_or_buffer)
    cur = container.Cursor(container.unframe(blob, MAGIC, VERSION, "zstream"), "zstream", ITEMS)
    settings = container.read_settings(cur)
    if not isinstance(settings, dict):
        raise ValueError("zstream: the settings header is not a JSON object")
    lengths, records, words, total = qstream.parse_section(cur, SECTION, check_settings("zstream", settings))
    cur.end("the bit string")
    zeros = book_section(cur, settings, records, total, words.size)
    return ZStream(settings, lengths, records, words), container.budget(cur, len(blob)), len(blob), zeros


def read(path_or_buffer):
    """-> ZStream(settings, lengths, records, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits, under the six items of qstream.info -- "symbol_bits" (the Huffman codes of all leaves written: what
    train_nerv_all._huffman_total_bits returns for the parsed histogram), "run_index", "grid_side" (here with every record's `kept`),
    "code_table" (266 bytes), "header", "padding" -- plus "total" = their sum = 8 * file size, the counts "n_records", "n_runs", "n_symbols"
    (elements, zeros included), "bytes", and "n_zero_elements", "n_zero_leaves", "zero_parse"."""
    zs, out, nbytes, zeros = _parse(path_or_buffer)
    out.update(total=8 * nbytes, n_records=len(zs.records), n_runs=int(sum(r.run_bits.size for r in zs.records)),
               n_symbols=int(sum(r.count for r in zs.records)), bytes=nbytes, n_zero_elements=int(zeros),
               n_zero_leaves=int(zs.settings["n_zero_leaves"]), zero_parse=zs.settings["zero_parse"])
    out.update(stored_frames_item(zs.settings))
    return out
