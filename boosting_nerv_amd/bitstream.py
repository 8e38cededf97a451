"""Container of a compressed video: what train_nerv_compression.evaluate() only counts, as a file.

Host-only code, little-endian throughout; framing, cursor, settings header, embedding header and raw section are container.py's
(DESIGN section 40):

    magic "BNRV" | version u32 | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings the model constructors read -- settings only, no code)
                n_tensors u32  | n_tensors x record                 (order of model._quant_modules(), weight before bias)
                n_embeds u32 | C u32 | h u32 | w u32 | n_embeds x (record + beta f32)     (HNeRV_Boost: one per frame; else all four 0)
                n_raw u32 | n_raw x (count u32 | count x f32)       (the decoder's state_dict entries no record covers, in its order)
    record  :=  count u32 | scale f32 | mean f32 | std f32 | lo i32 | hi i32 | n_words u32 | n_words x u32

`mean`, `std` (after the encoder's clamp), `lo` and `hi` parametrise the quantised Gaussian of the range-ANS coder (csrc/ans.cpp);
`scale` (and `beta` for an embedding) de-quantise the decoded symbols.  read() raises ValueError for a bad magic number, an unknown
version, a truncated file or a CRC mismatch; info() itemises where every bit of the file went."""
import struct
from collections import namedtuple

import numpy as np

from . import container
from .container import F32 as _F32, U32 as _U32

MAGIC = b"BNRV"
VERSION = 1
_RECORD = struct.Struct("<IfffiiI")       # count, scale, mean, std, lo, hi, n_words
ITEMS = ("tensor_words", "tensor_side", "embed_words", "embed_side", "raw", "header")

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


def to_bytes(settings, tensors, embeds=(), embed_shape=None, raw=()):
    tensors, embeds = list(tensors), list(embeds)
    out = [container.header_bytes(settings), _U32.pack(len(tensors))]
    for r in tensors:
        _pack_record(out, r, False)
    out.append(container.embed_head_bytes("bitstream", embeds, embed_shape))
    for r in embeds:
        _pack_record(out, r, True)
    out.append(container.raw_bytes(list(raw)))
    return container.frame(MAGIC, VERSION, b"".join(out))


def write(path_or_buffer, settings, tensors, embeds=(), embed_shape=None, raw=()):
    """Write a bitstream; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, tensors, embeds, embed_shape, raw))


def _read_record(cur, with_beta, side, coded):
    count, scale, mean, std, lo, hi, n_words = (cur.unpack(_RECORD, side))
    beta = cur.array("<f4", 1, side)[0] if with_beta else None
    words = cur.array("<u4", n_words, coded)
    if hi < lo:
        raise ValueError(f"bitstream: a record's symbol range [{lo}, {hi}] is empty")
    # (struct gives Python floats: back to the float32 values that were written, bit for bit)
    return Record(count, _f32(scale), _f32(mean), _f32(std), lo, hi, words, beta)


def _parse(path_or_buffer):
    blob = container.blob_of(path_or_buffer)
    cur = container.Cursor(container.unframe(blob, MAGIC, VERSION, "bitstream"), "bitstream", ITEMS)
    settings = container.read_settings(cur)                # (any JSON value: what the header must say is the decoder's business)
    n_tensors, = cur.unpack(_U32, "header")
    tensors = [_read_record(cur, False, "tensor_side", "tensor_words") for _ in range(n_tensors)]
    n_embeds, embed_shape = container.read_embed_head(cur)
    embeds = [_read_record(cur, True, "embed_side", "embed_words") for _ in range(n_embeds)]
    raw = container.read_raw(cur)
    cur.end("the last section")
    return Bitstream(settings, tensors, embeds, embed_shape, raw), container.budget(cur, len(blob)), len(blob)


def read(path_or_buffer):
    """-> Bitstream(settings, tensors, embeds, embed_shape, raw).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def info(path_or_buffer):
    """The bit budget of a file: {"tensor_words", "tensor_side", "embed_words", "embed_side", "raw", "header"} in bits -- the ANS words
    of the weight / bias tensors, their per-tensor side information (count, scale, mean, std, lo, hi, word count), the same two for the
    frame embeddings (side information: + beta), the raw fp32 section, and the header with the container's framing (magic, version,
    lengths, section counts, CRC) -- plus "coded_words" = tensor_words + embed_words, "total" = the sum of the six items = 8 * file size,
    and the counts "n_tensors", "n_embeds", "n_raw", "bytes"."""
    bs, out, nbytes = _parse(path_or_buffer)
    out.update(coded_words=out["tensor_words"] + out["embed_words"], total=8 * nbytes, n_tensors=len(bs.tensors), n_embeds=len(bs.embeds),
               n_raw=len(bs.raw), bytes=nbytes)
    return out
