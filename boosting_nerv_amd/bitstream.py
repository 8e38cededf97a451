"""Container of a compressed video: what train_nerv_compression.evaluate() only counts, as a file.

Host-only code, little-endian throughout:

    magic "BNRV" | version u32 | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings the model constructors read -- settings only, no code)
                n_tensors u32  | n_tensors x record                 (order of model._quant_modules(), weight before bias)
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (record + beta f32)     (HNeRV_Boost: one per frame; else all four 0)
                n_raw u32 | n_raw x (count u32 | count x f32)       (the decoder's state_dict entries no record covers, in its order)
    record  :=  count u32 | scale f32 | mean f32 | std f32 | lo i32 | hi i32 | n_words u32 | n_words x u32

`mean`, `std` (after the encoder's clamp), `lo` and `hi` parametrise the quantised Gaussian of the range-ANS coder (csrc/ans.cpp);
`scale` (and `beta` for an embedding) de-quantise the decoded symbols.  read() raises ValueError for a bad magic number, an unknown
version, a truncated file or a CRC mismatch; info() itemises where every bit of the file went."""
import io
import json
import struct
import zlib
from collections import namedtuple

import numpy as np

MAGIC = b"BNRV"
VERSION = 1
_PREFIX = struct.Struct("<4sIQ")          # magic, version, payload length
_RECORD = struct.Struct("<IfffiiI")       # count, scale, mean, std, lo, hi, n_words
_U32 = struct.Struct("<I")
_F32 = struct.Struct("<f")

Record = namedtuple("Record", "count scale mean std lo hi words beta", defaults=(None,))
Record.__doc__ = """One coded tensor.  scale / mean / std / beta: np.float32 (beta: None for a weight or bias);  words: uint32 array."""
Bitstream = namedtuple("Bitstream", "settings tensors embeds embed_shape raw")
Bitstream.__doc__ = """settings: dict;  tensors / embeds: [Record];  embed_shape: (C, h, w) or None;  raw: [float32 array]"""


def _f32(v):
    return np.float32(v)


def _pack_record(out, r, with_beta):
    words = np.ascontiguousarray(r.words, dtype="<u4")
    out.append(_RECORD.pack(int(r.count), _f32(r.scale), _f32(r.mean), _f32(r.std), int(r.lo), int(r.hi), words.size))
    if with_beta:
        out.append(_F32.pack(_f32(r.beta)))
    out.append(words.tobytes())


def _payload(settings, tensors, embeds, embed_shape, raw):
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    out = [_U32.pack(len(header)), header, _U32.pack(len(tensors))]
    for r in tensors:
        _pack_record(out, r, False)
    if embeds and embed_shape is None:
        raise ValueError("bitstream.write: embedding records need embed_shape (C, h, w)")
    out.append(struct.pack("<IIII", len(embeds), *(embed_shape if embeds else (0, 0, 0))))
    for r in embeds:
        _pack_record(out, r, True)
    out.append(_U32.pack(len(raw)))
    for a in raw:
        a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
        out.append(_U32.pack(a.size))
        out.append(a.tobytes())
    return b"".join(out)


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=()):
    """Write a bitstream; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    payload = _payload(settings, list(tensors), list(embeds), embed_shape, list(raw))
    blob = _PREFIX.pack(MAGIC, VERSION, len(payload)) + payload + _U32.pack(zlib.crc32(payload) & 0xFFFFFFFF)
    if hasattr(path_or_buffer, "write"):
        path_or_buffer.write(blob)
    else:
        with open(path_or_buffer, "wb") as f:
            f.write(blob)
    return len(blob)


def _blob(path_or_buffer):
    if isinstance(path_or_buffer, (bytes, bytearray, memoryview)):
        return bytes(path_or_buffer)
    if hasattr(path_or_buffer, "getvalue"):
        return path_or_buffer.getvalue()
    if hasattr(path_or_buffer, "read"):
        return path_or_buffer.read()
    with open(path_or_buffer, "rb") as f:
        return f.read()


class _Cursor:
    """Bounds-checked reads of the payload; `bits` books every byte it hands out under the name of a budget item."""

    def __init__(self, data):
        self.data, self.pos, self.bits = data, 0, {}

    def take(self, n, item):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError(f"bitstream: truncated ({item} needs {n} bytes at offset {self.pos} of a {len(self.data)}-byte payload)")
        piece = self.data[self.pos:self.pos + n]
        self.pos += n
        self.bits[item] = self.bits.get(item, 0) + 8 * n
        return piece

    def unpack(self, st, item):
        return st.unpack(self.take(st.size, item))


def _read_record(cur, with_beta, side, coded):
    count, scale, mean, std, lo, hi, n_words = (cur.unpack(_RECORD, side))
    beta = np.frombuffer(cur.take(4, side), dtype="<f4")[0] if with_beta else None
    words = np.frombuffer(cur.take(4 * n_words, coded), dtype="<u4").astype(np.uint32)
    if hi < lo:
        raise ValueError(f"bitstream: a record's symbol range [{lo}, {hi}] is empty")
    # (struct gives Python floats: back to the float32 values that were written, bit for bit)
    return Record(count, _f32(scale), _f32(mean), _f32(std), lo, hi, words, beta)


def _parse(path_or_buffer):
    blob = _blob(path_or_buffer)
    if len(blob) < _PREFIX.size:
        raise ValueError(f"bitstream: truncated ({len(blob)} bytes: shorter than the file prefix)")
    magic, version, length = _PREFIX.unpack_from(blob)
    if magic != MAGIC:
        raise ValueError(f"bitstream: bad magic number {magic!r} (want {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"bitstream: unknown format version {version} (this build reads version {VERSION})")
    if len(blob) != _PREFIX.size + length + 4:
        raise ValueError(f"bitstream: truncated or padded ({len(blob)} bytes, the prefix announces {_PREFIX.size + length + 4})")
    payload = blob[_PREFIX.size:_PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != _U32.unpack_from(blob, _PREFIX.size + length)[0]:
        raise ValueError("bitstream: CRC mismatch (the payload is damaged)")
    cur = _Cursor(payload)
    n_header, = cur.unpack(_U32, "header")
    try:
        settings = json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"bitstream: the settings header is not JSON ({e})") from None
    n_tensors, = cur.unpack(_U32, "header")
    tensors = [_read_record(cur, False, "tensor_side", "tensor_words") for _ in range(n_tensors)]
    n_embeds, C_, h_, w_ = cur.unpack(struct.Struct("<IIII"), "header")
    embeds = [_read_record(cur, True, "embed_side", "embed_words") for _ in range(n_embeds)]
    n_raw, = cur.unpack(_U32, "header")
    raw = []
    for _ in range(n_raw):
        cnt, = cur.unpack(_U32, "raw")
        raw.append(np.frombuffer(cur.take(4 * cnt, "raw"), dtype="<f4").astype(np.float32))
    if cur.pos != len(payload):
        raise ValueError(f"bitstream: {len(payload) - cur.pos} payload bytes follow the last section")
    cur.bits["header"] += 8 * (_PREFIX.size + 4)           # magic, version, length and the CRC
    return Bitstream(settings, tensors, embeds, (C_, h_, w_) if n_embeds else None, raw), cur.bits, len(blob)


def read(path_or_buffer):
    """-> Bitstream(settings, tensors, embeds, embed_shape, raw).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file: {"tensor_words", "tensor_side", "embed_words", "embed_side", "raw", "header"} in bits -- the ANS words
    of the weight / bias tensors, their per-tensor side information (count, scale, mean, std, lo, hi, word count), the same two for the
    frame embeddings (side information: + beta), the raw fp32 section, and the header with the container's framing (magic, version,
    lengths, section counts, CRC) -- plus "coded_words" = tensor_words + embed_words, "total" = the sum of the six items = 8 * file size,
    and the counts "n_tensors", "n_embeds", "n_raw", "bytes"."""
    bs, bits, nbytes = _parse(path_or_buffer)
    out = {k: int(bits.get(k, 0)) for k in ("tensor_words", "tensor_side", "embed_words", "embed_side", "raw", "header")}
    total = sum(out.values())
    assert total == 8 * nbytes, (total, nbytes)            # every byte was booked exactly once
    out.update(coded_words=out["tensor_words"] + out["embed_words"], total=total, n_tensors=len(bs.tensors), n_embeds=len(bs.embeds),
               n_raw=len(bs.raw), bytes=nbytes)
    return out


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=()):
    buf = io.BytesIO()
    write(buf, settings, tensors, embeds, embed_shape, raw)
    return buf.getvalue()
