"""CPU suite (``-m "not gpu"``) of the wide chunked CEM file: the host coder of records that span more than 4096 symbol
values, the BNRW container, the host repack and the surface."""
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import ROOT
from wstream_cases import RUNS, SIZES, SPANS, TOTAL, check_word_bound, min_shift, record, slot_words, tables, version1_blob

NEW_SYMBOLS = ("bnerv_ans_gaussian_bucket_cdf", "bnerv_ans_encode_wide_runs", "bnerv_ans_decode_wide_runs", "bnerv_sym_hist_wide",
               "bnerv_rans_encode_wide", "bnerv_rans_dequant_wide")


# ---------------------------------------------------------------------------------------------------------------------- host coder
def test_the_spans_take_the_shifts_the_format_names():
    from boosting_nerv_amd import wstream
    assert [min_shift(s) for s in SPANS] == [1, 1, 2, 3, 9] and [wstream.min_shift(0, s - 1) for s in SPANS] == [1, 1, 2, 3, 9]
    assert [wstream.min_shift(-5, -5 + s - 1) for s in (2, 4096, 1 << 23, (1 << 23) + 1, 1 << 28)] == [0, 0, 11, 12, 16]
    # a last bucket that holds one value only, on every span but 8192
    assert [(s - 1) % (1 << min_shift(s)) == 0 for s in SPANS] == [True, False, True, True, True]


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("span", SPANS)
def test_wide_runs_round_trip_within_the_word_bound(span, run):
    """Every size under both models; lo and hi are among the symbols (hi alone in a record of one)."""
    from boosting_nerv_amd.lib import entropy_model as em
    for n in SIZES:
        sym, lo, hi, k = record(span, n, 1000 * n + run)
        assert hi in sym and (n == 1 or lo in sym) and k == min_shift(span) > 0
        for model, cdf in enumerate(tables(sym, lo, hi, k)):
            assert cdf.size - 1 == -(-span // (1 << k)) <= 4096 and cdf[-1] == TOTAL
            words, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, run)
            assert rw.dtype == np.uint16 and rw.size == -(-n // run) and int(rw.sum()) == words.size, (n, model)
            check_word_bound(rw, n, run, k)
            got = em.ans_decode_wide_runs(words, rw, n, lo, hi, cdf, k, run)
            assert got.dtype == np.int32 and np.array_equal(got, sym), (n, model)


@pytest.mark.parametrize("run", RUNS)
def test_with_shift_0_the_words_are_those_of_the_table_runs_and_the_cdf_is_the_gaussian_cdf(run):
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(run)
    for span, n in ((2, 5), (61, 4097), (4096, 9000)):
        lo = int(rng.integers(-4000, 4000))
        hi = lo + span - 1
        sym = np.clip(np.rint(rng.normal((lo + hi) / 2, span / 6, size=n)), lo, hi).astype(np.int32)
        mean, std = float(np.float32(sym.mean())), float(np.float32(sym.std()))
        g = em.ans_gaussian_bucket_cdf(lo, hi, 0, mean, std)
        assert np.array_equal(g, em.ans_gaussian_cdf(lo, hi, mean, std))
        for cdf in (g, em.ans_counts_cdf(np.bincount(sym - lo, minlength=span))):
            want_w, want_rw = em.ans_encode_table_runs(sym, lo, cdf, run)
            got_w, got_rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, 0, run)
            assert np.array_equal(got_w, want_w) and np.array_equal(got_rw, want_rw)
            assert np.array_equal(em.ans_decode_wide_runs(got_w, got_rw, n, lo, hi, cdf, 0, run), sym)


def test_the_longest_message_fits_its_slot_and_its_u16_count():
    """A one-slot bucket with every raw bit, repeated for a whole run of 4096 at shift 11: 35 bits a symbol."""
    from boosting_nerv_amd.lib import entropy_model as em
    lo, hi, k, run = -(1 << 22), (1 << 22) - 1, 11, 4096
    assert min_shift(hi - lo + 1) == k
    counts = np.zeros(4096, np.uint32)
    counts[0] = 1_000_000
    cdf = em.ans_counts_cdf(counts)
    assert cdf[8] - cdf[7] == 1
    for low in (0, (1 << k) - 1):
        sym = np.full(run, lo + (7 << k) + low, np.int32)
        words, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, run)
        assert rw.tolist() == [words.size] and run * 35 // 32 <= words.size <= slot_words(run, k) == 4483 < 65536
        assert np.array_equal(em.ans_decode_wide_runs(words, rw, run, lo, hi, cdf, k, run), sym)
    assert slot_words(4096, 16) == 5123 < 65536               # the largest slot the format admits


def test_the_host_decoder_refuses_damaged_input():
    from boosting_nerv_amd._lib import BnervError
    from boosting_nerv_amd.lib import entropy_model as em
    sym, lo, hi, k = record(25457, 700, 3)
    cdf = tables(sym, lo, hi, k)[1]
    words, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, 256)
    assert rw.size == 3
    flipped = words.copy()
    flipped[int(rw[0]) + 5] ^= 0x00010000                     # a word of the second run
    with pytest.raises(BnervError, match="run 1"):
        em.ans_decode_wide_runs(flipped, rw, 700, lo, hi, cdf, k, 256)
    short = rw.copy()
    short[0] -= 1
    short[1] += 1                                             # the sum holds; the first run has lost a word to the second
    with pytest.raises(BnervError, match="run 0"):
        em.ans_decode_wide_runs(words, short, 700, lo, hi, cdf, k, 256)
    with pytest.raises(BnervError, match="add up"):
        em.ans_decode_wide_runs(words[:-1], rw, 700, lo, hi, cdf, k, 256)
    # a low part that lands past hi: coded on a range one value longer (the same buckets), decoded on the true one
    s2, lo2, hi2, k2 = record(4097, 65, 4)
    cdf2 = tables(s2, lo2, hi2, k2)[0]
    assert (hi2 + 1 - lo2) >> k2 == (hi2 - lo2) >> k2         # hi + 1 lies in the last bucket too
    past = s2.copy()
    past[40] = hi2 + 1
    w2, rw2 = em.ans_encode_wide_runs(past, lo2, hi2 + 1, cdf2, k2, 64)
    assert np.array_equal(em.ans_decode_wide_runs(w2, rw2, 65, lo2, hi2 + 1, cdf2, k2, 64), past)
    with pytest.raises(BnervError, match="run 0"):
        em.ans_decode_wide_runs(w2, rw2, 65, lo2, hi2, cdf2, k2, 64)
    # and the encoder refuses a symbol outside the range, a table that does not match it, a shift the format does not have
    with pytest.raises(BnervError, match="outside"):
        em.ans_encode_wide_runs(past, lo2, hi2, cdf2, k2, 64)
    with pytest.raises(BnervError, match="buckets"):
        em.ans_encode_wide_runs(s2, lo2, hi2, cdf2, k2 + 1, 64)
    with pytest.raises(BnervError, match="buckets"):
        em.ans_decode_wide_runs(w2, rw2, 65, lo2, hi2, cdf2[:-1], k2, 64)
    with pytest.raises(BnervError, match="bad model"):
        em.ans_gaussian_bucket_cdf(0, 100000, 17, 0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------- container
_cache = {}


def _files(tables_):
    """(version-1 bytes with a 25 457-value record, its BNRW bytes at run 64, symbols)."""
    if tables_ not in _cache:
        from boosting_nerv_amd import codec
        v1, symbols = _cache.setdefault("v1", version1_blob(True))
        w = io.BytesIO()
        codec.repack(v1, w, 64, tables=tables_, wide=True)
        _cache[tables_] = (v1, w.getvalue(), symbols)
    return _cache[tables_]


@pytest.mark.parametrize("tables_", ["gaussian", "empirical"])
def test_write_read_info_round_trip_and_the_budget_adds_up(tmp_path, tables_):
    from boosting_nerv_amd import codec, estream, wstream
    v1, blob, symbols = _files(tables_)
    assert blob[:4] == b"BNRW"
    ws = wstream.read(blob)
    assert ws.settings["ans_wide"] is True and ws.settings["ans_tables"] == tables_ and ws.settings["ans_run"] == 64
    assert [r.shift for r in ws.tensors + ws.embeds] == [3, 0, 0, 0, 0, 0] and ws.embed_shape == (2, 4, 5)
    for k, sym in enumerate(symbols):
        assert np.array_equal(wstream.decode_record(ws, k), sym), k
    if tables_ == "gaussian":
        assert all(r.model == estream.GAUSSIAN for r in ws.tensors + ws.embeds)
    else:
        assert ws.tensors[0].model == estream.TABLE and ws.tensors[0].freq.size == 3183       # the clustered record takes its bucket table
    again = wstream.to_bytes(ws.settings, ws.tensors, ws.embeds, ws.embed_shape, ws.raw, ws.words)
    assert again == blob
    path = tmp_path / "x.bnrw"
    assert wstream.write(str(path), ws.settings, ws.tensors, ws.embeds, ws.embed_shape, ws.raw, ws.words) == len(blob) and path.read_bytes() == blob
    budget = wstream.info(blob)
    assert budget == codec.info(blob) == wstream.info(str(path))
    assert budget["total"] == 8 * len(blob) == sum(budget[k] for k in estream.ITEMS) and budget["bytes"] == len(blob)
    assert budget["n_wide_records"] == 1 and budget["max_shift"] == 3 and budget["n_tensors"] == 3 and budget["n_embeds"] == 3
    # the side of a record: count, scale, lo, hi, model byte, SHIFT byte (+ mean, std under a Gaussian; + beta for an embedding)
    n_gauss_t = sum(r.model == estream.GAUSSIAN for r in ws.tensors)
    assert budget["tensor_side"] == 8 * (18 * 3 + 8 * n_gauss_t)
    assert "wide: 1 records" in codec.describe_any(budget) and "largest shift 3" in codec.describe_any(budget)
    print(f"{tables_}: version-1 {len(v1)} bytes, BNRW {len(blob)} bytes at run 64")


def _reframe(payload):
    from boosting_nerv_amd import rstream, wstream
    return rstream._PREFIX.pack(wstream.MAGIC, wstream.VERSION, len(payload)) + bytes(payload) + struct.pack("<I", zlib.crc32(bytes(payload)) & 0xFFFFFFFF)


def test_read_refusals():
    from boosting_nerv_amd import bitstream, estream, rstream, wstream
    v1, blob, symbols = _files("empirical")
    ws = wstream.read(blob)
    # ---- where estream.read refuses
    for other in (b"BNRV", b"BNRC", b"BNRE"):
        with pytest.raises(ValueError, match="magic"):
            wstream.read(other + blob[4:])
    for reader in (bitstream.read, rstream.read, estream.read):
        with pytest.raises(ValueError, match="magic"):
            reader(blob)                                      # and the older readers refuse the new kind
    with pytest.raises(ValueError, match="version"):
        wstream.read(blob[:4] + struct.pack("<I", 2) + blob[8:])
    for cut in (3, 15, len(blob) // 2, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated"):
            wstream.read(blob[:cut])
    flipped = bytearray(blob)
    flipped[len(blob) // 2] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        wstream.read(bytes(flipped))
    p = bytearray(blob[rstream._PREFIX.size:-4])
    n_header = struct.unpack_from("<I", p, 0)[0]
    rec0 = 4 + n_header + 4                                   # the first record: the one of 25 457 values under its table
    r0 = ws.tensors[0]
    assert r0.model == estream.TABLE and r0.shift == 3 and struct.unpack_from("<IfiiBB", p, rec0)[2:] == (r0.lo, r0.hi, 1, 3)
    runs0 = rec0 + 18 + len(estream.table_bytes(r0.freq))
    assert struct.unpack_from("<H", p, runs0)[0] == r0.run_words[0]
    q = bytearray(p)
    struct.pack_into("<H", q, runs0, int(r0.run_words[0]) + 1)
    with pytest.raises(ValueError, match="add up"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<HH", q, runs0, 1, int(r0.run_words[0]) + int(r0.run_words[1]) - 1)
    with pytest.raises(ValueError, match="two state words"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<I", q, rec0, 0)
    with pytest.raises(ValueError, match="0 symbols"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    q[-1] = 1
    with pytest.raises(ValueError, match="not zero"):
        wstream.read(_reframe(q))
    with pytest.raises(ValueError, match="follow"):
        wstream.read(_reframe(p + b"\0\0\0\0"))
    q = bytearray(p)
    q[rec0 + 16] = 2
    with pytest.raises(ValueError, match="model byte"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    q[rec0 + 18] ^= 1                                         # the first LEB128 value, one slot more or less: the sum breaks
    with pytest.raises(ValueError, match="sum to"):
        wstream.read(_reframe(q))
    j = int(np.flatnonzero(r0.freq - 1 < 0x80)[0])            # a one-byte value (a bucket no symbol fell into)
    at = rec0 + 18 + len(estream.table_bytes(r0.freq[:j]))
    assert p[at] == r0.freq[j] - 1
    q = bytearray(p)
    q[at:at + 1] = bytes([p[at] | 0x80, 0])                   # the same value padded with an empty last byte
    with pytest.raises(ValueError, match="padded"):
        wstream.read(_reframe(q))
    for bad in (0, 32, 100, 8192, "64", None):
        with pytest.raises(ValueError, match="run length"):
            wstream.to_bytes(dict(ws.settings, ans_run=bad), ws.tensors, ws.embeds, ws.embed_shape, ws.raw, ws.words)
    # ---- what this kind adds
    for s in (dict(ws.settings, ans_wide=False), {k: v for k, v in ws.settings.items() if k != "ans_wide"}, dict(ws.settings, ans_wide=1)):
        with pytest.raises(ValueError, match="ans_wide"):
            wstream.to_bytes(s, ws.tensors, ws.embeds, ws.embed_shape, ws.raw, ws.words)
    with pytest.raises(ValueError, match="ans_tables"):
        wstream.to_bytes(dict(ws.settings, ans_tables="laplace"), ws.tensors, ws.embeds, ws.embed_shape, ws.raw, ws.words)
    header = bytes(p[4:4 + n_header])
    assert b'"ans_wide":true' in header
    q = bytearray(p)
    q[4:4 + n_header] = header.replace(b'"ans_wide":true', b'"ans_wide":null')
    with pytest.raises(ValueError, match="ans_wide"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    q[rec0 + 17] = 4                                          # a shift that is not the minimal one: the same content would have two spellings
    with pytest.raises(ValueError, match="minimal"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    rec1 = runs0 + 2 * r0.run_words.size                      # the second record: 300 symbols on a narrow range, shift 0
    assert struct.unpack_from("<I", q, rec1)[0] == 300 and q[rec1 + 17] == 0
    q[rec1 + 17] = 1
    with pytest.raises(ValueError, match="minimal"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    q[rec0 + 17] = 17
    with pytest.raises(ValueError, match=r"shift is 17 \(0\.\.16\)"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<ii", q, rec1 + 8, 5, 5)                # one value: a table of one bucket
    with pytest.raises(ValueError, match="at least 2"):
        wstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<ii", q, rec1 + 8, 5, 4)
    with pytest.raises(ValueError, match="range"):
        wstream.read(_reframe(q))
    # write refuses what read refuses
    with pytest.raises(ValueError, match="minimal"):
        wstream.to_bytes(ws.settings, [r0._replace(shift=4)] + ws.tensors[1:], ws.embeds, ws.embed_shape, ws.raw, ws.words)
    with pytest.raises(ValueError, match="frequencies"):
        wstream.to_bytes(ws.settings, [r0._replace(freq=r0.freq[:-1])] + ws.tensors[1:], ws.embeds, ws.embed_shape, ws.raw, ws.words)


# ---------------------------------------------------------------------------------------------------------------------- repack
@pytest.mark.parametrize("tables_", ["gaussian", "empirical"])
def test_repack_wide_of_a_narrow_file_has_the_words_of_the_narrow_kinds_and_one_byte_more_per_record(tables_):
    from boosting_nerv_amd import codec, estream, rstream, wstream
    v1, symbols = version1_blob(False)
    run = 256
    w, e = io.BytesIO(), io.BytesIO()
    budget = codec.repack(v1, w, run, tables=tables_, wide=True)
    codec.repack(v1, e, run, tables=tables_)
    ws = wstream.read(w.getvalue())
    assert budget == wstream.info(w.getvalue()) and budget["n_wide_records"] == 0 and budget["max_shift"] == 0
    assert all(r.shift == 0 for r in ws.tensors + ws.embeds)
    n_rec = len(ws.tensors) + len(ws.embeds)
    if tables_ == "empirical":
        es = estream.read(e.getvalue())
        assert e.getvalue()[:4] == b"BNRE" and np.array_equal(ws.words, es.words)
        assert len(w.getvalue()) - len(e.getvalue()) == n_rec + len(b',"ans_wide":true')     # the shift byte of every record; the header says what kind it is
        for a, b in zip(ws.tensors + ws.embeds, es.tensors + es.embeds):
            assert a.model == b.model and np.array_equal(a.run_words, b.run_words) and (a.freq is None or np.array_equal(a.freq, b.freq))
        assert budget["tensor_side"] + budget["embed_side"] == estream.info(e.getvalue())["tensor_side"] + estream.info(e.getvalue())["embed_side"] + 8 * n_rec
    else:
        rs = rstream.read(e.getvalue())
        assert e.getvalue()[:4] == b"BNRC" and np.array_equal(ws.words, rs.words)
        assert all(r.model == estream.GAUSSIAN for r in ws.tensors + ws.embeds)
    for k, sym in enumerate(symbols):
        assert np.array_equal(wstream.decode_record(ws, k), sym)


@pytest.mark.parametrize("tables_", ["gaussian", "empirical"])
def test_repack_wide_of_a_wide_file_where_the_narrow_kinds_refuse(tmp_path, tables_):
    from boosting_nerv_amd import codec
    v1, blob, symbols = _files(tables_)
    with pytest.raises(NotImplementedError, match="wide"):
        codec.repack(v1, io.BytesIO(), 64, tables=tables_)                                    # today's raise sites stay
    with pytest.raises(ValueError, match="magic"):
        codec.repack(blob, io.BytesIO(), 64, tables=tables_, wide=True)                       # a BNRW file is no source
    with pytest.raises(ValueError, match="tables"):
        codec.repack(v1, io.BytesIO(), 64, tables="laplace", wide=True)
    # the command line, files by name
    src, dst = tmp_path / "in.bnrv", tmp_path / "out.bnrw"
    src.write_bytes(v1)
    budget = codec.main(["repack", str(src), str(dst), "--run", "64", "--tables", tables_, "--wide"])
    assert dst.read_bytes() == blob and codec.main(["info", str(dst)]) == budget
    # another run: the same symbols
    from boosting_nerv_amd import wstream
    other = io.BytesIO()
    codec.repack(v1, other, 4096, tables=tables_, wide=True)
    ws = wstream.read(other.getvalue())
    assert all(np.array_equal(wstream.decode_record(ws, k), s) for k, s in enumerate(symbols))


def test_repack_wide_from_a_chunked_file_gives_the_bytes_of_the_version_1_source():
    from boosting_nerv_amd import codec
    v1, _ = version1_blob(False)
    c, a, b = io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.repack(v1, c, 1024)
    codec.repack(v1, a, 256, tables="empirical", wide=True)
    codec.repack(c.getvalue(), b, 256, tables="empirical", wide=True)
    assert a.getvalue() == b.getvalue()


# ---------------------------------------------------------------------------------------------------------------------- surface
def test_flags_and_parser_errors():
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_compression as C
    p = C.build_parser()
    assert p.get_default("bitstream_wide") is False and p.parse_args(["--bitstream_wide", "--bitstream_run", "256"]).bitstream_wide is True
    with pytest.raises(SystemExit):
        C.main(["--bitstream", "x.bnrw", "--bitstream_wide"])                                 # N = 0: refused by the parser, before anything is built
    with pytest.raises(SystemExit):
        C.main(["--bitstream", "x.bnrw", "--bitstream_wide", "--bitstream_run", "0", "--bitstream_tables", "gaussian"])
    a = codec.build_parser().parse_args(["repack", "a", "b"])
    assert a.wide is False and codec.build_parser().parse_args(["repack", "a", "b", "--wide"]).wide is True
    with pytest.raises(ValueError, match="run > 0"):
        codec.encode(None, None, None, None, io.BytesIO(), wide=True)                         # refused before the model is looked at
    with pytest.raises(ValueError, match="run > 0"):
        codec.encode(None, None, None, None, io.BytesIO(), run=0, tables="empirical", wide=True)


def test_header_declares_the_new_entry_points_and_the_abi_version_stays():
    import ctypes as C
    from boosting_nerv_amd import _lib, ops, wstream
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    assert int(re.search(r"#define\s+BNERV_RANSW_MAX_SHIFT\s+(\d+)", header).group(1)) == _lib.RANSW_MAX_SHIFT == wstream.MAX_SHIFT == 16
    assert C.sizeof(_lib.WsymItem) == 32 and C.sizeof(_lib.RanswItem) == 48
    assert C.sizeof(_lib.HistItem) == 24 and C.sizeof(_lib.RencItem) == 24 and C.sizeof(_lib.RansItem) == 40      # the narrow items are not widened
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.bnerv_abi_version() == 9
    assert all(callable(f) for f in (ops.sym_hist_wide, ops.SymHistWide, ops.AnsEncodeRunsWide, ops.AnsDequantWide, ops.ans_dequant_wide))
    assert issubclass(ops.AnsDequantWide, ops.AnsDequant) and issubclass(ops.AnsEncodeRunsWide, ops.AnsEncodeRuns)
    for m in ("launch", "check", "run_words", "compact", "result"):
        assert callable(getattr(ops.AnsEncodeRunsWide, m))
    # the launchers validate before they touch a device
    assert lib.bnerv_sym_hist_wide(None, None, 0, None, 0, None, 0, None) != 0
    assert lib.bnerv_rans_encode_wide(None, None, 0, None, 0, None, 0, 64, None, 0, 51, None, None) != 0
    assert lib.bnerv_rans_dequant_wide(None, None, 0, None, 0, None, 0, None, 0, None, 0, 64, None) != 0
    with pytest.raises(ValueError, match="no items"):
        ops.AnsDequantWide(np.zeros(2, np.uint32), [], 64)
    with pytest.raises(ValueError, match="no items"):
        ops.AnsEncodeRunsWide([], 64)
    with pytest.raises(ValueError, match="no items"):
        ops.SymHistWide([])
