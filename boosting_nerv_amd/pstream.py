"""Container of a post-hoc quantised model whose frame embeddings are coded in time: the tensors as a qstream file
 or a zstream file holds them, the [N, C, h, w] embedding tensor frame by frame, every frame either
as its 8-bit codes q_t ("intra") or as the differences d_t = (q_t - q_{t-1}) mod 256 to the frame before ("inter"), the two kinds under
Huffman codes of their own.  The quantisation is untouched: a decoder rebuilds the very codes hnerv_utils.quant_tensor produced.

Host-only code (numpy and struct), little-endian throughout; framing, cursor and settings header are container.py's, the tensor section is written and
parsed by qstream.py's section functions under the name of this module:

    magic "BNRP" | version u32 | payload length u64 | payload | CRC32(payload) u32

    payload :=  header length u32 | header (UTF-8 JSON: the settings of a qstream header -- of a zstream header when tensor_kind is "sparse" --
                                            plus embed_pred "prev" and tensor_kind "dense" | "sparse")
                tensor section            (byte for byte what qstream / zstream write behind their header for the records WITHOUT the
                                           embedding record: 257 | 266 code lengths, n_records u32 and the records, n_words u32 and the words)
                embedding section
    embedding section :=
                N u32 | C u32 | h u32 | w u32
                outer u32 | red u32 | inner u32 | dtype u32 (0 fp32, 1 fp16) | outer * inner x min | outer * inner x scale
                                          (ONE grid: quant_tensor's for the whole [N, C, h, w] tensor, as in a qstream record)
                257 x u8 intra code lengths | 257 x u8 inter code lengths     (all zero: the file has no inter frame)
                N x u8 pred               (0 intra, 1 inter)
                N * ceil(P / huff_run) x u16      (bit length of every run, frame by frame; P = C * h * w)
                n_words u32 | n_words x u32       (the runs of all intra frames back to back)
                n_words u32 | n_words x u32       (the runs of all inter frames back to back)

A frame is one item of the Huffman coder: its P symbols are cut into runs of huff_run, the last one may be shorter, a run never spans two
frames.  The symbols of an inter frame are (q_t - q_{t-1}) mod 256 whatever --quant_embed_bit is; a decoder computes q_t = (q_{t-1} + d_t) mod
256.  Element i = t * P + p of the tensor de-quantises with the (min, scale) pair of slice (i // (red * inner)) * inner + i % inner.

read() raises ValueError on everything qstream.read (zstream.read for a sparse tensor section) refuses, and on a missing embed_pred or
tensor_kind, a pred byte above 1, pred[0] = 1, an inter frame in a file without an inter table, a grid that does not cover N * P elements
and run lengths that do not add up to the two strings.  info() books every bit of the file under one of ten items.

choose() is the rule by which an encoder decides every frame's kind; it only reads histograms, so the host and the device path of
codec.encode_posthoc(..., temporal=True) decide alike."""
from collections import namedtuple

import numpy as np

from . import container, qstream, zstream
from .container import U32 as _U32
from .qstream import F16, F32, RUN, magic_of, n_runs      # noqa: F401  (re-exported)

MAGIC = b"BNRP"
VERSION = 1
LEAVES = qstream.LEAVES
EMBED_PRED = "prev"
KINDS = ("dense", "sparse")
INTRA, INTER = 0, 1
EMBED_ITEMS = ("embed_symbol_bits", "embed_run_index", "embed_side", "embed_tables")
ITEMS = qstream.ITEMS + EMBED_ITEMS
_SHAPE = container.EMBED_HEAD             # N, C, h, w
_GRID = container.EMBED_HEAD              # outer, red, inner, dtype

PEmbeds = namedtuple("PEmbeds", "shape outer red inner dtype min scale lengths0 lengths1 pred run_bits words0 words1")
PEmbeds.__doc__ = """The embedding section.  shape: (N, C, h, w);  outer / red / inner / dtype / min / scale: the grid, as in a qstream.QRecord;
lengths0 / lengths1: uint8 [257] intra and inter code lengths (lengths1 all zero: no inter frame);  pred: uint8 [N];  run_bits: uint16
[N, ceil(P / huff_run)];  words0 / words1: uint32 arrays, the intra and the inter bit string."""
PStream = namedtuple("PStream", "settings lengths records words embeds")
PStream.__doc__ = """settings: dict;  lengths / records / words: the tensor section, as in a QStream (tensor_kind "dense") or a ZStream ("sparse");
embeds: PEmbeds"""


def symbols(q):
    """What an encoder codes, from the uint8 codes q [N, P]: (d, h0, h1) with d[t] = (q[t] - q[t-1]) mod 256 (row 0 zero), h0[t] the 256-bin
    histogram of q[t] and h1[t] that of d[t] (h1[0] zero), int64 [N, 256] each -- the numpy form of ops.EmbedDeltaU8."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    if q.ndim != 2 or q.size == 0:
        raise ValueError(f"pstream: the codes of the embeddings must be a non-empty [N, P] array, got {q.shape}")
    d = np.zeros_like(q)
    d[1:] = q[1:] - q[:-1]                                 # (uint8 arithmetic wraps mod 256)
    h0 = np.stack([np.bincount(row, minlength=256) for row in q]).astype(np.int64)
    h1 = np.stack([np.bincount(row, minlength=256) for row in d]).astype(np.int64)
    h1[0] = 0
    return d, h0, h1


def string_words(hist, lengths):
    """The 32-bit words of the bit string that holds the symbols counted in `hist` (int64 [256]) under the code `lengths`."""
    return (int((np.asarray(hist, dtype=np.int64) * np.asarray(lengths[:256], dtype=np.int64)).sum()) + 31) // 32


def section_bits(n_frames, count, words0, words1, run=RUN):
    """The bits of an embedding section that change with the choice of the frames' kinds or scale with the clip: the two bit strings as they
    are written (whole words), the run index, both code tables and the pred bytes.  (Shape, grid and the two word counts are the same for
    every choice.)"""
    return 32 * (int(words0) + int(words1)) + 16 * int(n_frames) * n_runs(count, run) + 8 * 2 * LEAVES + 8 * int(n_frames)


def all_intra_section_bits(q, run=RUN):
    """section_bits of the codes q [N, P] with every frame on its own under ONE code: what no written section may exceed."""
    from .codec import huffman_lengths
    q = np.asarray(q, dtype=np.uint8)
    hist = np.bincount(q.reshape(-1), minlength=256)
    return section_bits(q.shape[0], q.shape[1], string_words(hist, huffman_lengths(hist)), 0, run)


def choose(h0, h1, count=None, run=RUN):
    """The kind of every frame from histograms alone (integers only) -> (pred uint8 [N], lengths0, lengths1); lengths1 is all zero when no frame
    is inter.  h0[t]: the histogram of q[t]; h1[t]: that of d[t] (row 0 is not read).

    1. trial codes: L0 = huffman_lengths(sum_t h0[t]), L1 = huffman_lengths(sum_{t >= 1} h1[t])   (codec.huffman_lengths, EOF leaf included)
    2. frame t >= 1 is inter iff sum_s h1[t][s] * L1[s] < sum_s h0[t][s] * L0[s]; a tie is intra
    3. ONE pass: L0 rebuilt from the intra frames' h0, L1 from the inter frames' h1
    4. if the section of that assignment (section_bits) is not strictly smaller than the all-intra section, every frame is intra
    so a written embedding section is never larger than the all-intra section of the same clip."""
    from .codec import huffman_lengths
    h0, h1 = np.asarray(h0, dtype=np.int64), np.asarray(h1, dtype=np.int64)
    if h0.ndim != 2 or h0.shape[1] != 256 or h1.shape != h0.shape or h0.shape[0] == 0:
        raise ValueError(f"pstream.choose: histograms of shapes {h0.shape}, {h1.shape} (want two [N, 256] arrays)")
    n = h0.shape[0]
    count = int(h0[0].sum()) if count is None else int(count)
    none = np.zeros(LEAVES, dtype=np.uint8)
    all0 = huffman_lengths(h0.sum(axis=0))
    pred = np.zeros(n, dtype=np.uint8)
    if n == 1:
        return pred, all0, none
    trial1 = huffman_lengths(h1[1:].sum(axis=0))
    cost0 = (h0 * all0[:256].astype(np.int64)).sum(axis=1)
    cost1 = (h1 * trial1[:256].astype(np.int64)).sum(axis=1)
    pred[1:] = cost1[1:] < cost0[1:]
    if not pred.any():
        return pred, all0, none
    inter = pred != 0
    l0, l1 = huffman_lengths(h0[~inter].sum(axis=0)), huffman_lengths(h1[inter].sum(axis=0))
    mixed = section_bits(n, count, string_words(h0[~inter].sum(axis=0), l0), string_words(h1[inter].sum(axis=0), l1), run)
    if mixed < section_bits(n, count, string_words(h0.sum(axis=0), all0), 0, run):
        return pred, l0, l1
    return np.zeros(n, dtype=np.uint8), all0, none


def _embed_section(e):
    n, c, h, w = (int(v) for v in e.shape)
    out = [_SHAPE.pack(n, c, h, w), _GRID.pack(int(e.outer), int(e.red), int(e.inner), int(e.dtype))] + qstream.grid_bytes("pstream", e, "grid")
    for ln in (e.lengths0, e.lengths1):
        ln = np.ascontiguousarray(ln, dtype=np.uint8)
        if ln.size != LEAVES:
            raise ValueError(f"pstream.write: a code table needs {LEAVES} lengths, got {ln.size}")
        out.append(ln.tobytes())
    pred = np.ascontiguousarray(e.pred, dtype=np.uint8)
    rb = np.ascontiguousarray(e.run_bits, dtype="<u2")
    if pred.size != n or rb.size % n:
        raise ValueError(f"pstream.write: {pred.size} pred bytes and {rb.size} run lengths for {n} frames")
    out += [pred.tobytes(), rb.tobytes()]
    for words in (e.words0, e.words1):
        wd = np.ascontiguousarray(words, dtype="<u4")
        out += [_U32.pack(wd.size), wd.tobytes()]
    return out


def to_bytes(settings, lengths, records, words, embeds):
    kind = settings.get("tensor_kind")
    if kind not in KINDS or settings.get("embed_pred") != EMBED_PRED:
        raise ValueError(f"pstream.write: the settings need embed_pred = {EMBED_PRED!r} and tensor_kind in {KINDS}")
    fmt = zstream if kind == "sparse" else qstream
    return container.frame(MAGIC, VERSION, b"".join(qstream._header(settings) + fmt._section(lengths, list(records), words) + _embed_section(embeds)))


def write(path_or_buffer, settings, lengths, records, words, embeds):
    """Write a file; returns the number of bytes written.  path_or_buffer: a file name or a binary file object."""
    return container.write_blob(path_or_buffer, to_bytes(settings, lengths, records, words, embeds))


def _parse_embeds(cur, run):
    n, c, h, w = cur.unpack(_SHAPE, "embed_side")
    count = c * h * w
    if n == 0 or count == 0:
        raise ValueError(f"pstream: an embedding tensor of shape ({n}, {c}, {h}, {w})")
    outer, red, inner, dtype = cur.unpack(_GRID, "embed_side")
    if dtype not in (F32, F16) or outer * red * inner != n * count:
        raise ValueError(f"pstream: {n} frames of {count} elements with the grid ({outer}, {red}, {inner}) of dtype flag {dtype}")
    lo, step = qstream.read_grid(cur, outer, inner, dtype, "embed_side")
    lengths0 = cur.array(np.uint8, LEAVES, "embed_tables")
    lengths1 = cur.array(np.uint8, LEAVES, "embed_tables")
    qstream.check_lengths(lengths0, who="pstream")
    if lengths1.any():
        qstream.check_lengths(lengths1, who="pstream")
    pred = cur.array(np.uint8, n, "embed_side")
    if int(pred.max()) > 1:
        raise ValueError(f"pstream: a pred byte of {int(pred.max())} (0 intra, 1 inter)")
    if pred[0] != INTRA:
        raise ValueError("pstream: frame 0 is coded as a difference (pred[0] = 1): there is no frame before it")
    if pred.any() and not lengths1.any():
        raise ValueError(f"pstream: {int(pred.sum())} frames are coded as differences, the inter code table is absent")
    per = n_runs(count, run)
    run_bits = cur.array("<u2", n * per, "embed_run_index").reshape(n, per)
    strings, bits = [], []
    for kind in (INTRA, INTER):
        n_words, = cur.unpack(_U32, "embed_side")
        strings.append(cur.array("<u4", n_words, "embed_symbol_bits"))
        bits.append(int(run_bits[pred == kind].sum(dtype=np.uint64)))
    return PEmbeds((n, c, h, w), outer, red, inner, dtype, lo, step, lengths0, lengths1, pred, run_bits, strings[0], strings[1]), bits


def _parse(path_or_buffer):
    blob = container.blob_of(path_or_buffer)
    cur = container.Cursor(container.unframe(blob, MAGIC, VERSION, "pstream"), "pstream", ITEMS)
    settings = container.read_settings(cur)
    if not isinstance(settings, dict):
        raise ValueError("pstream: the settings header is not a JSON object")
    if settings.get("embed_pred") != EMBED_PRED:
        raise ValueError(f"pstream: the header's embed_pred is {settings.get('embed_pred')!r} (this build reads {EMBED_PRED!r})")
    kind = settings.get("tensor_kind")
    if kind not in KINDS:
        raise ValueError(f"pstream: the header's tensor_kind is {kind!r} ({' | '.join(KINDS)})")
    if kind == "sparse":
        run = zstream.check_settings("pstream", settings)
    else:
        run = settings.get("huff_run")
        if not isinstance(run, int) or not 1 <= run <= 2047:
            raise ValueError(f"pstream: the header's run length is {run!r}")
    lengths, records, words, total = qstream.parse_section(cur, zstream.SECTION if kind == "sparse" else qstream.SECTION, run)
    embeds, bits = _parse_embeds(cur, run)
    cur.end("the bit strings")
    zeros = None
    if kind == "sparse":
        zeros = zstream.book_section(cur, settings, records, total, words.size)
    else:
        qstream.book_section(cur, total, words.size)
    for b, wd, name in zip(bits, (embeds.words0, embeds.words1), ("intra", "inter")):
        if (b + 31) // 32 != wd.size:
            raise ValueError(f"pstream: the run lengths of the {name} frames add up to {b} bits, their bit string has {wd.size} words")
    cur.bits["embed_symbol_bits"] = sum(bits)
    cur.bits["padding"] += 32 * (embeds.words0.size + embeds.words1.size) - sum(bits)
    return PStream(settings, lengths, records, words, embeds), container.budget(cur, len(blob)), len(blob), zeros, bits


def read(path_or_buffer):
    """-> PStream(settings, lengths, records, words, embeds).  path_or_buffer: a file name, a binary file object or bytes."""
    return _parse(path_or_buffer)[0]


def embed_section_bits(embeds, run=RUN):
    """section_bits of a read embedding section: what the bound of choose() is stated in."""
    n, c, h, w = embeds.shape
    return section_bits(n, c * h * w, embeds.words0.size, embeds.words1.size, run)


def info(path_or_buffer):
    """The bit budget of a file, in bits: the six items of qstream.info for the tensor section and the container ("symbol_bits", "run_index",
    "grid_side", "code_table", "header", "padding" -- the zero bits that end all three bit strings), then "embed_symbol_bits" (the Huffman
    codes of all frames), "embed_run_index" (16 per run), "embed_side" (shape, grid, pred bytes, the two word counts) and "embed_tables"
    (2 x 257 bytes) -- plus "total" = their sum = 8 * file size, the counts "n_records", "n_runs", "n_symbols" (of the tensor section),
    "n_embed_symbols", "n_embed_runs", "n_inter_frames", "n_intra_frames", "intra_frame_bits", "inter_frame_bits" (the codes of all frames
    of a kind), "embed_section_bits" (section_bits: what choose() compares), "bytes", "tensor_kind", and for a sparse tensor section
    zstream.info's "n_zero_elements", "n_zero_leaves", "zero_parse"."""
    ps, out, nbytes, zeros, strings = _parse(path_or_buffer)
    e = ps.embeds
    n_inter = int(e.pred.sum())
    out.update(total=8 * nbytes, n_records=len(ps.records), n_runs=int(sum(r.run_bits.size for r in ps.records)),
               n_symbols=int(sum(r.count for r in ps.records)), n_embed_symbols=int(np.prod(e.shape)), n_embed_runs=int(e.run_bits.size),
               n_inter_frames=n_inter, n_intra_frames=int(e.pred.size) - n_inter, intra_frame_bits=strings[0], inter_frame_bits=strings[1],
               embed_section_bits=embed_section_bits(e, int(ps.settings["huff_run"])), bytes=nbytes, tensor_kind=ps.settings["tensor_kind"])
    if zeros is not None:
        out.update(n_zero_elements=int(zeros), n_zero_leaves=int(ps.settings["n_zero_leaves"]), zero_parse=ps.settings["zero_parse"])
    out.update(qstream.stored_frames_item(ps.settings))
    return out


def decode_embeds(ps):
    """The host oracle of the embedding section -> uint8 [N, P] codes q: both strings through the host Huffman decoder, then the chains
    q_t = (q_{t-1} + d_t) mod 256 of the inter frames."""
    from .lib.entropy_model import huff_decode
    e = ps.embeds
    n, count = int(e.shape[0]), int(np.prod(e.shape[1:]))
    run = int(ps.settings["huff_run"])
    sym = np.zeros((n, count), dtype=np.uint8)
    for kind, lengths, words in ((INTRA, e.lengths0, e.words0), (INTER, e.lengths1, e.words1)):
        rows = np.flatnonzero(e.pred == kind)
        if rows.size:
            sym[rows] = huff_decode(words, e.run_bits[rows].reshape(-1), [count] * rows.size, lengths, run).reshape(rows.size, count)
    for t in range(1, n):
        if e.pred[t] == INTER:
            sym[t] += sym[t - 1]                           # (uint8 arithmetic wraps mod 256)
    return sym
