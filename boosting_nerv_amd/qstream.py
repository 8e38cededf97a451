"""Container of a post-hoc quantised model: what train_nerv_all.evaluate() only counts -- the 8-bit codes of
hnerv_utils.quant_tensor under ONE Huffman code -- as a file that decodes to the frames the `quant_*` metrics scored.

Host-only code (numpy and struct), little-endian throughout; framing, cursor and settings header are container.py's.  This module
is also the home of the Huffman family's tensor section -- code table, records, bit string -- which zstream.py and pstream.py write and
parse through section_bytes(), parse_section() and book_section() with a Section of their own:

    magic "BNRQ" | version u32 | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings the model constructors read, full_data_length, final_size, crop_list,
                                            quant_model_bit, quant_embed_bit, huff_run -- settings only, no code)
                257 x u8 code length              (symbols 0..255, then the EOF leaf; 0 = unused)
                n_records u32 | n_records x record
                n_words u32 | n_words x u32       (the bit string)
    record  :=  count u32 | outer u32 | red u32 | inner u32 | dtype u32 (0 fp32, 1 fp16)
                outer * inner x min | outer * inner x scale         (in the dtype quant_tensor produced)
                ceil(count / huff_run) x u16      (bit length of every run)

Records come in the order train_nerv_all._huffman_report concatenates the tensors: for HNeRV and HNeRV_Boost the [N, C, h, w] frame
embeddings first, then every state_dict entry whose key lacks `encoder`, in state_dict order.  No names are stored.
Element i of a record de-quantises with the (min, scale) pair of slice (i // (red * inner)) * inner + i % inner; a grid of one pair is
(outer, red, inner) = (1, count, 1).

The code.  Canonical from the lengths: leaves ordered by (length, leaf index), the first code of the shortest length is 0, every next
leaf takes the previous code + 1 shifted left by the growth in length.  A code's bits enter the bit string most significant first; bit p
of the string is bit 31 - p % 32 of word p // 32.  The symbols of a record are cut into runs of huff_run = 256; the last run of a record
may be shorter, a run never spans two records, the string is continuous over runs and records and padded with zero bits to the final word
only.  EOF is never written: the counts are stored.

read() raises ValueError for a bad magic number, an unknown version, a truncated file or a CRC mismatch (as bitstream.read does), and for
code lengths above 32 or off Kraft equality (over the used leaves, EOF among them) and run lengths that do not add up to the bit string.
info() books every bit of the file under one of six items."""
import struct
from collections import namedtuple

import numpy as np

from . import container
from .container import U32 as _U32, magic_of      # noqa: F401  (magic_of: re-exported)

MAGIC = b"BNRQ"
VERSION = 1
_PREFIX = container.PREFIX            # (the name the tests of the kinds frame their damaged payloads with)
RUN = 256                                 # BNERV_HUFF_RUN
LEAVES = 257
F32, F16 = 0, 1
_DTYPES = {F32: np.dtype("<f4"), F16: np.dtype("<f2")}
ITEMS = ("symbol_bits", "run_index", "grid_side", "code_table", "header", "padding")

QRecord = namedtuple("QRecord", "count outer red inner dtype min scale run_bits")
QRecord.__doc__ = """One quantised tensor.  dtype: F32 | F16;  min / scale: arrays of outer * inner entries in that dtype;  run_bits: uint16 array."""
QStream = namedtuple("QStream", "settings lengths records words")
QStream.__doc__ = """settings: dict;  lengths: uint8 [257];  records: [QRecord];  words: uint32 array (the bit string)"""
Section = namedtuple("Section", "who leaves record check")
Section.__doc__ = """A kind's tensor section.  who: the name in its writer's messages;  leaves: code lengths in its table;  record: its namedtuple -- QRecord's
fields, with further u32 fields (zstream: kept) behind dtype;  check(who, those fields): the kind's own refusal of a record, or None."""
SECTION = Section("qstream", LEAVES, QRecord, None)


def check_lengths(lengths, leaves=LEAVES, who="qstream"):
    """ValueError unless the `leaves` lengths describe a complete prefix code this family of formats carries."""
    ln = np.asarray(lengths)
    if ln.shape != (leaves,):
        raise ValueError(f"{who}: the code table needs {leaves} lengths, got {ln.shape}")
    if int(ln.max()) > 32:
        raise ValueError(f"{who}: a code length of {int(ln.max())} exceeds 32")
    used = [int(v) for v in ln if v]
    if not ln[leaves - 1] or sum(1 << (32 - v) for v in used) != 1 << 32:
        raise ValueError(f"{who}: the code lengths break Kraft equality over the used leaves and EOF")


def n_runs(count, run=RUN):
    return (int(count) + run - 1) // run


def _header(settings):
    return [container.header_bytes(settings)]


def grid_bytes(who, r, what):
    """The min and the scale array of a record or an embedding grid r, checked against its geometry and dtype flag; what: "record" | "grid"."""
    dt, out = _DTYPES[int(r.dtype)], []
    for a in (r.min, r.scale):
        a = np.asarray(a)
        if a.dtype != dt or a.size != int(r.outer) * int(r.inner):
            raise ValueError(f"{who}.write: a grid array of {a.size} {a.dtype} entries in a {what} of {int(r.outer) * int(r.inner)} {dt} slices")
        out.append(np.ascontiguousarray(a.reshape(-1)).astype(dt, copy=False).tobytes())
    return out


def read_grid(cur, outer, inner, dtype, item):
    """-> (min, scale) of outer * inner entries each."""
    return cur.array(_DTYPES[dtype], outer * inner, item), cur.array(_DTYPES[dtype], outer * inner, item)


def section_bytes(sec, lengths, records, words):
    """The payload behind the header -- code table, records, bit string -- as a list of byte strings."""
    head = struct.Struct(f"<{len(sec.record._fields) - 3}I")
    out = [np.ascontiguousarray(lengths, dtype=np.uint8).tobytes(), _U32.pack(len(records))]
    for r in records:
        out.append(head.pack(*(int(v) for v in r[:-3])))
        out += grid_bytes(sec.who, r, "record")
        out.append(np.ascontiguousarray(r.run_bits, dtype="<u2").tobytes())
    w = np.ascontiguousarray(words, dtype="<u4")
    out += [_U32.pack(w.size), w.tobytes()]
    return out


def parse_section(cur, sec, run):
    """What section_bytes wrote, read at the cursor -> (lengths, records, words, the bits the run lengths add up to)."""
    head = struct.Struct(f"<{len(sec.record._fields) - 3}I")
    lengths = cur.array(np.uint8, sec.leaves, "code_table")
    check_lengths(lengths, sec.leaves, cur.who)
    n_records, = cur.unpack(_U32, "header")
    records, total = [], 0
    for _ in range(n_records):
        fields = cur.unpack(head, "grid_side")
        count, outer, red, inner, dtype = fields[:5]
        if dtype not in _DTYPES or count == 0 or outer * red * inner != count:
            raise ValueError(f"{cur.who}: a record of {count} elements with the grid ({outer}, {red}, {inner}) of dtype flag {dtype}")
        if sec.check is not None:
            sec.check(cur.who, *fields)
        lo, step = read_grid(cur, outer, inner, dtype, "grid_side")
        run_bits = cur.array("<u2", n_runs(count, run), "run_index")
        total += int(run_bits.sum(dtype=np.uint64))
        records.append(sec.record(*fields, lo, step, run_bits))
    n_words, = cur.unpack(_U32, "header")
    return lengths, records, cur.array("<u4", n_words, "symbol_bits"), total


def book_section(cur, total, n_words):
    """The run lengths against the bit string; the string's bits booked as codes and padding."""
    if (total + 31) // 32 != n_words:
        raise ValueError(f"{cur.who}: the run lengths of the records add up to {total} bits, the bit string has {n_words} words")
    cur.bits["padding"] = 32 * n_words - total
    cur.bits["symbol_bits"] = total


def _section(lengths, records, words):
    return section_bytes(SECTION, lengths, records, words)


def to_bytes(settings, lengths, records, words):
    return container.frame(MAGIC, VERSION, b"".join(_header(settings) + _section(lengths, list(records), words)))


def write(path_or_buffer, settings, lengths, records, words):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, lengths, records, words))


def _parse(path_or_buffer):
    blob = container.blob_of(path_or_buffer)
    cur = container.Cursor(container.unframe(blob, MAGIC, VERSION, "qstream"), "qstream", ITEMS)
    settings = container.read_settings(cur)
    run = settings.get("huff_run") if isinstance(settings, dict) else None
    if not isinstance(run, int) or not 1 <= run <= 2047:
        raise ValueError(f"qstream: the header's run length is {run!r}")
    lengths, records, words, total = parse_section(cur, SECTION, run)
    cur.end("the bit string")
    book_section(cur, total, words.size)
    return QStream(settings, lengths, records, words), container.budget(cur, len(blob)), len(blob)


def read(path_or_buffer):
    """-> QStream(settings, lengths, records, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits: "symbol_bits" (the Huffman codes of all symbols: sum of count * code length, what
    train_nerv_all._huffman_total_bits returns), "run_index" (16 per run), "grid_side" (every record's count, grid geometry, dtype flag and
    its min / scale arrays), "code_table" (257 bytes), "header" (the JSON settings, the record and word counts and the container's framing:
    magic, version, length, CRC) and "padding" (zero bits up to the final word) -- plus "total" = their sum = 8 * file size, and the counts
    "n_records", "n_runs", "n_symbols", "bytes"."""
    qs, out, nbytes = _parse(path_or_buffer)
    out.update(total=8 * nbytes, n_records=len(qs.records), n_runs=int(sum(r.run_bits.size for r in qs.records)),
               n_symbols=int(sum(r.count for r in qs.records)), bytes=nbytes)
    out.update(stored_frames_item(qs.settings))
    return out


def stored_frames_item(settings):
    """{"n_stored_frames": S} for the header of an interpolation file (the key embed_stored = [N, a, b, c]; the embedding
    record holds S = embed_shape[0] of the N frames), {} for any other header.  A count, not a budget item: the bits are booked as ever."""
    if "embed_stored" not in settings:
        return {}
    shape = settings.get("embed_shape")
    if not isinstance(shape, list) or not shape or not isinstance(shape[0], int):
        raise ValueError(f"qstream: a header with embed_stored and the embedding shape {shape!r}")
    return {"n_stored_frames": int(shape[0])}
