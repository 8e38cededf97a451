"""Container of a SPARSE post-hoc quantised model: the twin of hnerv_utils.quant_tensor_sparse, in which a zero weight
stays exactly zero, under ONE Huffman code whose alphabet has leaves for zeros.  A sibling of qstream.py: the same
framing, JSON header, record order and grid geometry.

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
import io
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

from .qstream import F16, F32, ITEMS, RUN, _Cursor, _blob, _header, magic_of, n_runs, stored_frames_item     # noqa: F401  (the shared framing; re-exported)

MAGIC = b"BNRZ"
VERSION = 1
LEAVES = 266                              # BNERV_HUFFZ_LEAVES
ZERO = 256                                # BNERV_HUFFZ_ZERO: leaf ZERO + k is 2^k zero elements
ZERO_LEAVES = 9                           # BNERV_HUFFZ_ZERO_LEAVES
PARSES = ("single", "runs")               # BNERV_HUFFZ_SINGLE, BNERV_HUFFZ_RUNS, by index
_PREFIX = struct.Struct("<4sIQ")          # magic, version, payload length
_RECORD = struct.Struct("<IIIIII")        # count, outer, red, inner, dtype, kept
_U32 = struct.Struct("<I")
_DTYPES = {F32: np.dtype("<f4"), F16: np.dtype("<f2")}

ZRecord = namedtuple("ZRecord", "count outer red inner dtype kept min scale run_bits")
ZRecord.__doc__ = """One quantised tensor.  kept: its non-zero elements;  the rest as qstream.QRecord."""
ZStream = namedtuple("ZStream", "settings lengths records words")
ZStream.__doc__ = """settings: dict;  lengths: uint8 [266];  records: [ZRecord];  words: uint32 array (the bit string)"""


def check_lengths(lengths):
    """ValueError unless the 266 lengths describe a complete prefix code this format carries."""
    ln = np.asarray(lengths)
    if ln.shape != (LEAVES,):
        raise ValueError(f"zstream: the code table needs {LEAVES} lengths, got {ln.shape}")
    if int(ln.max()) > 32:
        raise ValueError(f"zstream: a code length of {int(ln.max())} exceeds 32")
    used = [int(v) for v in ln if v]
    if not ln[LEAVES - 1] or sum(1 << (32 - v) for v in used) != 1 << 32:
        raise ValueError("zstream: the code lengths break Kraft equality over the used leaves and EOF")


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
    """The payload behind the header -- code table, records, bit string -- as a list of byte strings (pstream.py holds the same bytes)."""
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    if ln.size != LEAVES:
        raise ValueError(f"zstream.write: the code table needs {LEAVES} lengths, got {ln.size}")
    out = [ln.tobytes(), _U32.pack(len(records))]
    for r in records:
        dt = _DTYPES[int(r.dtype)]
        out.append(_RECORD.pack(int(r.count), int(r.outer), int(r.red), int(r.inner), int(r.dtype), int(r.kept)))
        for a in (r.min, r.scale):
            a = np.asarray(a)
            if a.dtype != dt or a.size != int(r.outer) * int(r.inner):
                raise ValueError(f"zstream.write: a grid array of {a.size} {a.dtype} entries in a record of {int(r.outer) * int(r.inner)} {dt} slices")
            out.append(np.ascontiguousarray(a.reshape(-1)).astype(dt, copy=False).tobytes())
        out.append(np.ascontiguousarray(r.run_bits, dtype="<u2").tobytes())
    w = np.ascontiguousarray(words, dtype="<u4")
    out += [_U32.pack(w.size), w.tobytes()]
    return out


def _payload(settings, lengths, records, words):
    return b"".join(_header(settings) + _section(lengths, records, words))


def write(path_or_buffer, settings, lengths, records, words):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    payload = _payload(settings, lengths, list(records), words)
    blob = _PREFIX.pack(MAGIC, VERSION, len(payload)) + payload + _U32.pack(zlib.crc32(payload) & 0xFFFFFFFF)
    if hasattr(path_or_buffer, "write"):
        path_or_buffer.write(blob)
    else:
        with open(path_or_buffer, "wb") as f:
            f.write(blob)
    return len(blob)


def to_bytes(settings, lengths, records, words):
    buf = io.BytesIO()
    write(buf, settings, lengths, records, words)
    return buf.getvalue()


def _parse(path_or_buffer):
    blob = _blob(path_or_buffer)
    if len(blob) < _PREFIX.size:
        raise ValueError(f"zstream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != MAGIC:
        raise ValueError(f"zstream: bad magic number {magic!r} (want {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"zstream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"zstream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("zstream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    try:
        n_header, = cur.unpack(_U32, "header")
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"zstream: the settings header is not JSON ({e})") from None
    except ValueError as e:
        raise ValueError(str(e).replace("qstream", "zstream")) from None
    if not isinstance(settings, dict):
        raise ValueError("zstream: the settings header is not a JSON object")
    run = settings.get("huff_run")
    if not isinstance(run, int) or not 1 <= run <= RUN:
        raise ValueError(f"zstream: the header's run length is {run!r}")
    zero_leaves = settings.get("n_zero_leaves")
    if settings.get("zero_parse") not in PARSES or not isinstance(zero_leaves, int) or zero_leaves < 0:
        raise ValueError(f"zstream: the header's zero_parse / n_zero_leaves are {settings.get('zero_parse')!r} / {zero_leaves!r}")
    lengths, records, words, total, zeros = _parse_section(cur, run)
    if cur.pos != len(payload):
        raise ValueError(f"zstream: {len(payload) - cur.pos} payload bytes follow the bit string")
    _book_section(cur, settings, total, words.size, zeros)
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return ZStream(settings, lengths, records, words), cur.bits, len(blob), zeros


def _parse_section(cur, run):
    """What _section wrote, read at the cursor -> (lengths, records, words, the bits the run lengths add up to, the zero elements)."""
    try:
        lengths = np.frombuffer(cur.take(LEAVES, "code_table"), dtype=np.uint8).copy()
        check_lengths(lengths)
        n_records, = cur.unpack(_U32, "header")
        records, total, zeros = [], 0, 0
        for _ in range(n_records):
            count, outer, red, inner, dtype, kept = cur.unpack(_RECORD, "grid_side")
            if dtype not in _DTYPES or count == 0 or outer * red * inner != count:
                raise ValueError(f"zstream: a record of {count} elements with the grid ({outer}, {red}, {inner}) of dtype flag {dtype}")
            if kept > count:
                raise ValueError(f"zstream: a record of {count} elements announces {kept} kept ones")
            dt = _DTYPES[dtype]
            lo = np.frombuffer(cur.take(dt.itemsize * outer * inner, "grid_side"), dtype=dt).astype(dt.newbyteorder("="))
            step = np.frombuffer(cur.take(dt.itemsize * outer * inner, "grid_side"), dtype=dt).astype(dt.newbyteorder("="))
            run_bits = np.frombuffer(cur.take(2 * n_runs(count, run), "run_index"), dtype="<u2").astype(np.uint16)
            total += int(run_bits.sum(dtype=np.uint64))
            zeros += count - kept
            records.append(ZRecord(count, outer, red, inner, dtype, kept, lo, step, run_bits))
        n_words, = cur.unpack(_U32, "header")
        words = np.frombuffer(cur.take(4 * n_words, "symbol_bits"), dtype="<u4").astype(np.uint32)
    except ValueError as e:
        raise ValueError(str(e).replace("qstream", "zstream")) from None
    return lengths, records, words, total, zeros


def _book_section(cur, settings, total, n_words, zeros):
    """The run lengths against the bit string and the header's zero-run leaves against the records; the string's bits booked as codes and padding."""
    zero_leaves = settings["n_zero_leaves"]
    if (total + 31) // 32 != n_words:
        raise ValueError(f"zstream: the run lengths of the records add up to {total} bits, the bit string has {n_words} words")
    if zero_leaves > zeros or (zero_leaves == 0) != (zeros == 0) or (settings["zero_parse"] == "single" and zero_leaves != zeros):
        raise ValueError(f"zstream: the header announces {zero_leaves} zero-run leaves ({settings['zero_parse']}), the records hold {zeros} zero elements")
    cur.bits["padding"] = 32 * n_words - total
    cur.bits["symbol_bits"] = total


def read(path_or_buffer):
    """-> ZStream(settings, lengths, records, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits, under the six items of qstream.info -- "symbol_bits" (the Huffman codes of all leaves written: what
    train_nerv_all._huffman_total_bits returns for the parsed histogram), "run_index", "grid_side" (here with every record's `kept`),
    "code_table" (266 bytes), "header", "padding" -- plus "total" = their sum = 8 * file size, the counts "n_records", "n_runs", "n_symbols"
    (elements, zeros included), "bytes", and "n_zero_elements", "n_zero_leaves", "zero_parse"."""
    zs, bits, nbytes, zeros = _parse(path_or_buffer)
    out = {k: int(bits[k]) for k in ITEMS}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    out.update(total=total, n_records=len(zs.records), n_runs=int(sum(r.run_bits.size for r in zs.records)),
               n_symbols=int(sum(r.count for r in zs.records)), bytes=nbytes, n_zero_elements=int(zeros),
               n_zero_leaves=int(zs.settings["n_zero_leaves"]), zero_parse=zs.settings["zero_parse"])
    out.update(stored_frames_item(zs.settings))
    return out
