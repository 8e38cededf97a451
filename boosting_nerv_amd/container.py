"""What the eight kinds of file share ("One container layer"): the framing

    magic (4 bytes) | version u32 | payload length u64 | payload | CRC32(payload) u32

the bounds-checked cursor that books every payload byte under a budget item, the JSON settings header every payload opens with, the
raw fp32 section and the embedding header of the CEM kinds, and the epilogue of every bit budget.  Host-only code (numpy, struct, zlib,
json), little-endian throughout.  A reader passes `who`, the name its messages start with: no message is renamed afterwards."""
import json
import struct
import zlib

import numpy as np

PREFIX = struct.Struct("<4sIQ")           # magic, version, payload length
U32 = struct.Struct("<I")
F32 = struct.Struct("<f")
EMBED_HEAD = struct.Struct("<IIII")       # n_embeds, C, h, w
LEB128_MAX = 1 << 24                      # the largest value Cursor.leb128 hands out: the slots of a symbol table


def blob_of(src):
    """The bytes of a file.  src: a file name, a binary file object or bytes."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if hasattr(src, "getvalue"):
        return src.getvalue()
    if hasattr(src, "read"):
        return src.read()
    with open(src, "rb") as f:
        return f.read()


def magic_of(src):
    """The first four bytes of a file (codec.Decoder and the CLI dispatch on them); a file object is rewound."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src[:4])
    if hasattr(src, "getvalue"):
        return src.getvalue()[:4]
    if hasattr(src, "read"):
        at = src.tell()
        head = src.read(4)
        src.seek(at)
        return head
    with open(src, "rb") as f:
        return f.read(4)


def write_blob(dst, blob):
    """Write the bytes of a file; returns their number.  dst: a file name or a binary file object."""
    if hasattr(dst, "write"):
        dst.write(blob)
    else:
        with open(dst, "wb") as f:
            f.write(blob)
    return len(blob)


def frame(magic, version, payload):
    return PREFIX.pack(magic, version, len(payload)) + payload + U32.pack(zlib.crc32(payload) & 0xFFFFFFFF)


def unframe(blob, magic, version, who):
    """The payload of a file of the kind `magic`; ValueError for a short file, another magic number or version, a length that differs from
    the announced one and a CRC mismatch."""
    if len(blob) < PREFIX.size:
        raise ValueError(f"{who}: truncated ({len(blob)} bytes: shorter than the file prefix)")
    got, ver, length = PREFIX.unpack_from(blob)
    if got != magic:
        raise ValueError(f"{who}: bad magic number {got!r} (want {magic!r})")
    if ver != version:
        raise ValueError(f"{who}: unknown format version {ver} (this build reads version {version})")
    if len(blob) != PREFIX.size + length + 4:
        raise ValueError(f"{who}: truncated or padded ({len(blob)} bytes, the prefix announces {PREFIX.size + length + 4})")
    payload = blob[PREFIX.size:PREFIX.size + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != U32.unpack_from(blob, PREFIX.size + length)[0]:
        raise ValueError(f"{who}: CRC mismatch (the payload is damaged)")
    return payload


class Cursor:
    """Bounds-checked reads of the payload; `bits` books every byte it hands out under the name of a budget item (one of `items`)."""

    def __init__(self, data, who, items):
        self.data, self.who, self.pos, self.bits = data, who, 0, dict.fromkeys(items, 0)

    def take(self, n, item):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError(f"{self.who}: truncated ({item} needs {n} bytes at offset {self.pos} of a {len(self.data)}-byte payload)")
        piece = self.data[self.pos:self.pos + n]
        self.pos += n
        self.bits[item] += 8 * n
        return piece

    def unpack(self, st, item):
        return st.unpack(self.take(st.size, item))

    def array(self, dtype, n, item):
        """n values of the little-endian `dtype`, as a native array of their own."""
        dtype = np.dtype(dtype)
        return np.frombuffer(self.take(dtype.itemsize * n, item), dtype=dtype).astype(dtype.newbyteorder("="))

    def leb128(self, item):
        v, shift = 0, 0
        while True:
            if self.pos >= len(self.data):
                raise ValueError(f"{self.who}: truncated (a LEB128 value of {item} runs past the {len(self.data)}-byte payload)")
            b = self.data[self.pos]
            self.pos += 1
            self.bits[item] += 8
            v |= (b & 0x7F) << shift
            shift += 7
            if v > LEB128_MAX or shift > 28:               # (shift: a value padded with continuation bytes)
                raise ValueError(f"{self.who}: a LEB128 value of {item} exceeds 2^24")
            if not b & 0x80:
                if b == 0 and shift > 7:                   # one value, one spelling: the writer never ends on an empty group
                    raise ValueError(f"{self.who}: a LEB128 value of {item} is padded with an empty last byte")
                return v

    def end(self, after):
        """ValueError unless the payload ends here; after: what the last section is called."""
        if self.pos != len(self.data):
            raise ValueError(f"{self.who}: {len(self.data) - self.pos} payload bytes follow {after}")


def header_bytes(settings):
    """header length u32 | the settings as UTF-8 JSON (sorted keys, no spaces)."""
    header = json.dumps(settings, sort_keys=True, separators=(",", ":")).encode("utf-8")
    return U32.pack(len(header)) + header


def read_settings(cur):
    """What header_bytes wrote, as the JSON value it holds.  Whether anything but an object is refused is the kind's business."""
    n_header, = cur.unpack(U32, "header")
    try:
        return json.loads(cur.take(n_header, "header").decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"{cur.who}: the settings header is not JSON ({e})") from None


def raw_bytes(raw):
    """n_raw u32 | n_raw x (count u32 | count x f32)."""
    out = [U32.pack(len(raw))]
    for a in raw:
        a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
        out += [U32.pack(a.size), a.tobytes()]
    return b"".join(out)


def read_raw(cur):
    n_raw, = cur.unpack(U32, "header")
    return [cur.array("<f4", cur.unpack(U32, "raw")[0], "raw") for _ in range(n_raw)]


def embed_head_bytes(who, embeds, embed_shape):
    """n_embeds u32 | C u32 | h u32 | w u32 (all four 0 without embedding records)."""
    if embeds and embed_shape is None:
        raise ValueError(f"{who}.write: embedding records need embed_shape (C, h, w)")
    return EMBED_HEAD.pack(len(embeds), *(embed_shape if embeds else (0, 0, 0)))


def read_embed_head(cur):
    """-> (n_embeds, (C, h, w) or None)."""
    n_embeds, *shape = cur.unpack(EMBED_HEAD, "header")
    return n_embeds, tuple(shape) if n_embeds else None


def budget(cur, nbytes):
    """The epilogue of a parse: the framing (magic, version, length and the CRC) joins "header", and every byte of the file of `nbytes`
    bytes was booked exactly once.  -> {item: bits}, in the order of the cursor's items."""
    cur.bits["header"] += 8 * (PREFIX.size + 4)
    out = {k: int(v) for k, v in cur.bits.items()}
    assert sum(out.values()) == 8 * nbytes, (out, nbytes)
    return out
