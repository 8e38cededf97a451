"""Container of a post-hoc quantised model: what train_nerv_all.evaluate() only counts -- the 8-bit codes of
hnerv_utils.quant_tensor under ONE Huffman code -- as a file that decodes to the frames the `quant_*` metrics scored.

Host-only code (numpy and struct), little-endian throughout; the framing is bitstream.py's:

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
import io
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

MAGIC = b"BNRQ"
VERSION = 1
RUN = 256                                 # BNERV_HUFF_RUN
LEAVES = 257
F32, F16 = 0, 1
_PREFIX = struct.Struct("<4sIQ")          # magic, version, payload length
_RECORD = struct.Struct("<IIIII")         # count, outer, red, inner, dtype
_U32 = struct.Struct("<I")
_DTYPES = {F32: np.dtype("<f4"), F16: np.dtype("<f2")}
ITEMS = ("symbol_bits", "run_index", "grid_side", "code_table", "header", "padding")

QRecord = namedtuple("QRecord", "count outer red inner dtype min scale run_bits")
QRecord.__doc__ = """One quantised tensor.  dtype: F32 | F16;  min / scale: arrays of outer * inner entries in that dtype;  run_bits: uint16 array."""
QStream = namedtuple("QStream", "settings lengths records words")
QStream.__doc__ = """settings: dict;  lengths: uint8 [257];  records: [QRecord];  words: uint32 array (the bit string)"""


def check_lengths(lengths):
    """ValueError unless the 257 lengths describe a complete prefix code this format carries."""
    ln = np.asarray(lengths)
    if ln.shape != (LEAVES,):
        raise ValueError(f"qstream: the code table needs {LEAVES} lengths, got {ln.shape}")
    if int(ln.max()) > 32:
        raise ValueError(f"qstream: a code length of {int(ln.max())} exceeds 32")
    used = [int(v) for v in ln if v]
    if not ln[LEAVES - 1] or sum(1 << (32 - v) for v in used) != 1 << 32:
        raise ValueError("qstream: the code lengths break Kraft equality over the used leaves and EOF")


def n_runs(count, run=RUN):
    return (int(count) + run - 1) // run


def _header(settings):
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    return [_U32.pack(len(header)), header]


def _section(lengths, records, words):
    """The payload behind the header -- code table, records, bit string -- as a list of byte strings (pstream.py holds the same bytes)."""
    ln = np.ascontiguousarray(lengths, dtype=np.uint8)
    out = [ln.tobytes(), _U32.pack(len(records))]
    for r in records:
        dt = _DTYPES[int(r.dtype)]
        out.append(_RECORD.pack(int(r.count), int(r.outer), int(r.red), int(r.inner), int(r.dtype)))
        for a in (r.min, r.scale):
            a = np.asarray(a)
            if a.dtype != dt or a.size != int(r.outer) * int(r.inner):
                raise ValueError(f"qstream.write: a grid array of {a.size} {a.dtype} entries in a record of {int(r.outer) * int(r.inner)} {dt} slices")
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


def _blob(path_or_buffer):
    if isinstance(path_or_buffer, (bytes, bytearray, memoryview)):
        return bytes(path_or_buffer)
    if hasattr(path_or_buffer, "getvalue"):
        return path_or_buffer.getvalue()
    if hasattr(path_or_buffer, "read"):
        return path_or_buffer.read()
    with open(path_or_buffer, "rb") as f:
        return f.read()


def magic_of(path_or_buffer):
    """The first four bytes of a file (codec.Decoder and the CLI dispatch on them); a file object is rewound."""
    if isinstance(path_or_buffer, (bytes, bytearray, memoryview)):
        return bytes(path_or_buffer[:4])
    if hasattr(path_or_buffer, "getvalue"):
        return path_or_buffer.getvalue()[:4]
    if hasattr(path_or_buffer, "read"):
        at = path_or_buffer.tell()
        head = path_or_buffer.read(4)
        path_or_buffer.seek(at)
        return head
    with open(path_or_buffer, "rb") as f:
        return f.read(4)


class _Cursor:
    """Bounds-checked reads of the payload; `bits` books every byte it hands out under the name of a budget item."""

    def __init__(self, data):
        self.data, self.pos, self.bits = data, 0, dict.fromkeys(ITEMS, 0)

    def take(self, n, item):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError(f"qstream: truncated ({item} needs {n} bytes at offset {self.pos} of a {len(self.data)}-byte payload)")
        piece = self.data[self.pos:self.pos + n]
        self.pos += n
        self.bits[item] += 8 * n
        return piece

    def unpack(self, st, item):
        return st.unpack(self.take(st.size, item))


def _parse(path_or_buffer):
    blob = _blob(path_or_buffer)
    if len(blob) < _PREFIX.size:
        raise ValueError(f"qstream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != MAGIC:
        raise ValueError(f"qstream: bad magic number {magic!r} (want {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"qstream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"qstream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("qstream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    n_header, = cur.unpack(_U32, "header")
    try:
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"qstream: the settings header is not JSON ({e})") from None
    run = settings.get("huff_run") if isinstance(settings, dict) else None
    if not isinstance(run, int) or not 1 <= run <= 2047:
        raise ValueError(f"qstream: the header's run length is {run!r}")
    lengths, records, words, total = _parse_section(cur, run)
    if cur.pos != len(payload):
        raise ValueError(f"qstream: {len(payload) - cur.pos} payload bytes follow the bit string")
    _book_section(cur, total, words.size)
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return QStream(settings, lengths, records, words), cur.bits, len(blob)


def _parse_section(cur, run):
    """What _section wrote, read at the cursor -> (lengths, records, words, the bits the run lengths add up to)."""
    lengths = np.frombuffer(cur.take(LEAVES, "code_table"), dtype=np.uint8).copy()
    check_lengths(lengths)
    n_records, = cur.unpack(_U32, "header")
    records, total = [], 0
    for _ in range(n_records):
        count, outer, red, inner, dtype = cur.unpack(_RECORD, "grid_side")
        if dtype not in _DTYPES or count == 0 or outer * red * inner != count:
            raise ValueError(f"qstream: a record of {count} elements with the grid ({outer}, {red}, {inner}) of dtype flag {dtype}")
        dt = _DTYPES[dtype]
        lo = np.frombuffer(cur.take(dt.itemsize * outer * inner, "grid_side"), dtype=dt).astype(dt.newbyteorder("="))
        step = np.frombuffer(cur.take(dt.itemsize * outer * inner, "grid_side"), dtype=dt).astype(dt.newbyteorder("="))
        run_bits = np.frombuffer(cur.take(2 * n_runs(count, run), "run_index"), dtype="<u2").astype(np.uint16)
        total += int(run_bits.sum(dtype=np.uint64))
        records.append(QRecord(count, outer, red, inner, dtype, lo, step, run_bits))
    n_words, = cur.unpack(_U32, "header")
    words = np.frombuffer(cur.take(4 * n_words, "symbol_bits"), dtype="<u4").astype(np.uint32)
    return lengths, records, words, total


def _book_section(cur, total, n_words):
    """The run lengths against the bit string; the string's bits booked as codes and padding."""
    if (total + 31) // 32 != n_words:
        raise ValueError(f"qstream: the run lengths of the records add up to {total} bits, the bit string has {n_words} words")
    cur.bits["padding"] = 32 * n_words - total
    cur.bits["symbol_bits"] = total


def read(path_or_buffer):
    """-> QStream(settings, lengths, records, words).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file, in bits: "symbol_bits" (the Huffman codes of all symbols: sum of count * code length, what
    train_nerv_all._huffman_total_bits returns), "run_index" (16 per run), "grid_side" (every record's count, grid geometry, dtype flag and
    its min / scale arrays), "code_table" (257 bytes), "header" (the JSON settings, the record and word counts and the container's framing:
    magic, version, length, CRC) and "padding" (zero bits up to the final word) -- plus "total" = their sum = 8 * file size, and the counts
    "n_records", "n_runs", "n_symbols", "bytes"."""
    qs, bits, nbytes = _parse(path_or_buffer)
    out = {k: int(bits[k]) for k in ITEMS}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    out.update(total=total, n_records=len(qs.records), n_runs=int(sum(r.run_bits.size for r in qs.records)),
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
