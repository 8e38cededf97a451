"""CPU suite (``-m "not gpu"``) of the temporal CEM file: the BNRT container, the moments of a difference record, the
choice rule of the host repack on clips of constructed symbols, and the surface."""
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import ROOT
from tstream_cases import CASES, EMBED_SHAPE, FAR, MODES, N_FRAMES, P, RUNS, TABLES, check_bound, delta_reference, hand_built, version1_blob

NEW_SYMBOLS = ("bnerv_embed_delta", "bnerv_rans_decode_wide", "bnerv_embed_chain_dequant")


def _repacked(name, run, tables, temporal=True):
    from boosting_nerv_amd import codec
    out = io.BytesIO()
    budget = codec.repack(version1_blob(CASES[name]()), out, run, tables, wide=True, temporal=temporal)
    return out.getvalue(), budget


def _reframe(payload):
    from boosting_nerv_amd import rstream, tstream
    return rstream._PREFIX.pack(tstream.MAGIC, tstream.VERSION, len(payload)) + bytes(payload) + struct.pack("<I", zlib.crc32(bytes(payload)) & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------- container
@pytest.mark.parametrize("tables", TABLES)
def test_write_read_info_round_trip_and_the_budget_adds_up(tmp_path, tables):
    from boosting_nerv_amd import codec, tstream, wstream
    blob, budget = _repacked("black", 64, tables)
    assert blob[:4] == b"BNRT" and codec.info(blob) == budget == tstream.info(blob)
    ts = tstream.read(blob)
    assert ts.settings["embed_pred"] == "prev" and ts.settings["ans_wide"] is True and ts.settings["ans_run"] == 64
    assert ts.embed_shape == EMBED_SHAPE and len(ts.embeds) == len(ts.preds) == N_FRAMES and all(r.count == P for r in ts.embeds)
    # written again from what was read: the same bytes, to a file and to a buffer
    again = tstream.to_bytes(ts.settings, ts.tensors, ts.embeds, ts.preds, ts.embed_shape, ts.raw, ts.words)
    assert again == blob
    path = str(tmp_path / "clip.bnrt")
    assert tstream.write(path, ts.settings, ts.tensors, ts.embeds, ts.preds, ts.embed_shape, ts.raw, ts.words) == len(blob) == os.path.getsize(path)
    assert open(path, "rb").read() == blob and tstream.info(path) == budget
    # every bit under one of estream's eight items; the pred byte is embedding side
    from boosting_nerv_amd.estream import ITEMS
    assert sum(budget[k] for k in ITEMS) == budget["total"] == 8 * len(blob) == 8 * budget["bytes"]
    wide_blob, wide_budget = _repacked("black", 64, tables, temporal=False)
    intra = [k for k, p in enumerate(ts.preds) if p == 0]
    assert budget["n_inter_frames"] + budget["n_intra_frames"] == N_FRAMES == budget["n_embeds"] and budget["n_intra_frames"] == len(intra)
    for k in ("n_tensors", "n_raw", "n_runs", "n_symbols", "ans_run", "ans_tables", "raw", "run_index", "padding", "tensor_side"):
        assert budget[k] == wide_budget[k], k
    # an intra record is the wide file's record, byte for byte
    ws = wstream.read(wide_blob)
    for k in intra:
        a, b = ts.embeds[k], ws.embeds[k]
        assert (a.lo, a.hi, a.model, a.shift, a.mean, a.std, a.beta) == (b.lo, b.hi, b.model, b.shift, b.mean, b.std, b.beta) and np.array_equal(a.run_words, b.run_words)
    assert "temporal: " in codec.describe_any(budget) and "wide: " in codec.describe_any(budget)


def test_read_refusals():
    from boosting_nerv_amd import bitstream, estream, rstream, tstream, wstream
    blob, _ = _repacked("walk", 64, "gaussian")
    ts = tstream.read(blob)
    assert ts.preds == [0, 1, 1, 1, 1, 1]
    # ---- where wstream.read refuses: magic, version, length, CRC
    for other in (b"BNRV", b"BNRC", b"BNRE", b"BNRW"):
        with pytest.raises(ValueError, match="magic"):
            tstream.read(other + blob[4:])
    for reader in (bitstream.read, rstream.read, estream.read, wstream.read):
        with pytest.raises(ValueError, match="magic"):
            reader(blob)                                      # and the older readers refuse the new kind
    with pytest.raises(ValueError, match="tstream: unknown format version"):
        tstream.read(blob[:4] + struct.pack("<I", 2) + blob[8:])
    for cut in (3, 15, len(blob) // 2, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated"):
            tstream.read(blob[:cut])
    flipped = bytearray(blob)
    flipped[len(blob) // 2] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        tstream.read(bytes(flipped))
    p = bytearray(blob[rstream._PREFIX.size:-4])
    with pytest.raises(ValueError, match="follow"):
        tstream.read(_reframe(p + b"\0\0\0\0"))
    # ---- the pred bytes: find the embedding section behind the tensor records (all Gaussian here: 18 + 8 bytes and the run lengths)
    assert all(r.model == estream.GAUSSIAN for r in ts.tensors + ts.embeds)
    at = 4 + struct.unpack_from("<I", p, 0)[0] + 4 + sum(26 + 2 * r.run_words.size for r in ts.tensors)
    assert struct.unpack_from("<IIII", p, at) == (N_FRAMES,) + EMBED_SHAPE
    pred0 = at + 16
    rec_bytes = 1 + 26 + 2 * ts.embeds[0].run_words.size + 4
    assert [p[pred0 + k * rec_bytes] for k in range(N_FRAMES)] == ts.preds
    q = bytearray(p)
    q[pred0 + rec_bytes] = 2
    with pytest.raises(ValueError, match="pred byte of frame 1 is 2"):
        tstream.read(_reframe(q))
    q = bytearray(p)
    q[pred0] = 1
    with pytest.raises(ValueError, match="frame 0 is predicted"):
        tstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<I", q, at + 4, EMBED_SHAPE[0] + 1)             # C + 1: no record has C * h * w symbols any more
    with pytest.raises(ValueError, match="576 symbols"):
        tstream.read(_reframe(q))
    # ---- the header
    for settings, what in ((dict(ts.settings, embed_pred="next"), "embed_pred"), ({k: v for k, v in ts.settings.items() if k != "embed_pred"}, "embed_pred"),
                           (dict(ts.settings, ans_wide=False), "ans_wide")):
        with pytest.raises(ValueError, match=what):
            tstream.to_bytes(settings, ts.tensors, ts.embeds, ts.preds, ts.embed_shape, ts.raw, ts.words)
        header = __import__("json").dumps(settings, sort_keys=True, separators=(",", ":")).encode()
        n0 = struct.unpack_from("<I", p, 0)[0]
        with pytest.raises(ValueError, match="tstream: .*" + what):
            tstream.read(_reframe(struct.pack("<I", len(header)) + header + bytes(p[4 + n0:])))
    # ---- a file without embedding records: nothing to predict
    n_words = sum(int(r.run_words.sum()) for r in ts.tensors)
    with pytest.raises(ValueError, match="nothing to predict"):
        tstream.to_bytes(ts.settings, ts.tensors, [], [], None, ts.raw, ts.words[:n_words])
    wide = rstream.payload(tstream.KIND, {k: v for k, v in ts.settings.items()}, ts.tensors, [], None, ts.raw, ts.words[:n_words])
    with pytest.raises(ValueError, match="nothing to predict"):
        tstream.read(_reframe(wide))
    # ---- the writer refuses what the reader would
    with pytest.raises(ValueError, match="frame 0 is predicted"):
        tstream.to_bytes(ts.settings, ts.tensors, ts.embeds, [1] + ts.preds[1:], ts.embed_shape, ts.raw, ts.words)
    with pytest.raises(ValueError, match="pred byte"):
        tstream.to_bytes(ts.settings, ts.tensors, ts.embeds, ts.preds[:-1] + [3], ts.embed_shape, ts.raw, ts.words)
    with pytest.raises(ValueError, match="pred bytes for"):
        tstream.to_bytes(ts.settings, ts.tensors, ts.embeds, ts.preds[:-1], ts.embed_shape, ts.raw, ts.words)


# ---------------------------------------------------------------------------------------------------------------------- moments
def test_delta_moments_against_float64_numpy():
    from boosting_nerv_amd import tstream
    rng = np.random.default_rng(0)
    for n, spread in ((2, 3), (576, 1), (576, 1 << 20), (4097, 700), (1 << 16, 1 << 20)):
        d = rng.integers(-spread, spread + 1, size=n)
        n_, s1, s2 = tstream.delta_sums(d)
        assert (n_, s1, s2) == (n, int(d.sum()), int((d.astype(object) ** 2).sum()))
        mean, std = tstream.delta_moments(n, s1, s2)
        assert mean.dtype == std.dtype == np.float32
        want_mean, want_std = d.astype(np.float64).mean(), d.astype(np.float64).std(ddof=1)
        assert mean == np.float32(s1 / n) and abs(float(mean) - want_mean) <= 2.0 ** -23 * max(abs(want_mean), 2.0 ** -100)
        assert abs(float(std) - want_std) <= 2.0 ** -22 * want_std          # float64's own error in the two-pass formula is far below fp32 rounding
    # a constant record: std 0, clamped to the coder's floor; n = 1 likewise
    for n, v in ((576, 0), (576, -7), (1, 5), (1, 0)):
        mean, std = tstream.delta_moments(*tstream.delta_sums(np.full(n, v)))
        assert mean == np.float32(v) and std == np.float32(1e-5)
    with pytest.raises(ValueError):
        tstream.delta_moments(0, 0, 0)
    assert tstream.eligible(1 << 24, -(1 << 20), 1 << 20)
    assert not tstream.eligible(576, -(1 << 20) - 1, 0) and not tstream.eligible(576, 0, (1 << 20) + 1) and not tstream.eligible((1 << 24) + 1, 0, 1)


# ---------------------------------------------------------------------------------------------------------------------- host repack
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_repack_temporal_codes_the_constructed_clips_as_the_rule_says(name, run, tables):
    from boosting_nerv_amd import tstream, wstream
    q = CASES[name]()
    blob, budget = _repacked(name, run, tables)
    wide_blob, wide_budget = _repacked(name, run, tables, temporal=False)
    ts, ws = tstream.read(blob), wstream.read(wide_blob)
    want = MODES[name]
    want = dict(enumerate(want)) if isinstance(want, list) else want
    assert ts.preds[0] == 0 and {t: ts.preds[t] for t in want} == want, ts.preds
    assert np.array_equal(tstream.decode_embeds(ts), q)
    check_bound(budget, wide_budget)
    n_t = len(ts.tensors)
    for t, pred in enumerate(ts.preds):                      # what every record holds: the frame, or its difference to the frame before
        held = tstream.decode_record(ts, n_t + t)
        assert np.array_equal(held, q[t] - q[t - 1] if pred else q[t])
        if pred:
            r = ts.embeds[t]
            d, lo, hi, s1, s2 = delta_reference(q)
            assert (r.lo, r.hi) == (int(lo[t]), max(int(hi[t]), int(lo[t]) + 1)) and (r.scale, r.beta) == (ws.embeds[t].scale, ws.embeds[t].beta)
            if r.model == 0:
                assert (r.mean, r.std) == tstream.delta_moments(P, int(s1[t]), int(s2[t]))
    if name == "independent":                                # every frame intra: the words are the wide file's words
        assert np.array_equal(ts.words, ws.words) and budget["n_inter_frames"] == 0
        assert budget["embed_side"] == wide_budget["embed_side"] + 8 * N_FRAMES and budget["ans_words"] == wide_budget["ans_words"]
    if name == "walk":
        assert budget["n_inter_frames"] == N_FRAMES - 1 and budget["ans_words"] < wide_budget["ans_words"] * 0.6
    if name == "far":                                        # the difference of frame 2 is a near-constant, and out of reach
        d = q[2].astype(np.int64) - q[1]
        assert int(d.min()) == FAR - 1 and int(d.max()) == FAR + 1 and not tstream.eligible(P, d.min(), d.max())


def test_repack_temporal_from_a_chunked_file_gives_the_bytes_of_the_version_1_source():
    from boosting_nerv_amd import codec
    v1 = version1_blob(CASES["black"]())
    chunked, a, b = io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.repack(v1, chunked, 128)
    codec.repack(chunked.getvalue(), a, 64, "empirical", wide=True, temporal=True)
    codec.repack(v1, b, 64, "empirical", wide=True, temporal=True)
    assert a.getvalue() == b.getvalue()


def test_decode_embeds_resolves_hand_built_chains_and_refuses_one_that_leaves_int32():
    from boosting_nerv_amd import tstream
    rng = np.random.default_rng(5)
    held = rng.integers(-40, 41, size=(5, P)).astype(np.int32)
    preds = [0, 1, 1, 0, 1]
    ts = tstream.read(hand_built(held, preds))
    want = held.astype(np.int64).copy()
    for t in (1, 2, 4):
        want[t] += want[t - 1]
    got = tstream.decode_embeds(ts)
    assert got.dtype == np.int32 and got.shape == (5, P) and np.array_equal(got, want)
    top = np.full(P, (1 << 31) - 10, np.int32)
    assert np.array_equal(tstream.decode_embeds(tstream.read(hand_built([top, np.full(P, 9, np.int32)], [0, 1])))[1], top + 9)      # 2^31 - 1: the last value
    with pytest.raises(ValueError, match="leaves int32"):
        tstream.decode_embeds(tstream.read(hand_built([top, np.full(P, 10, np.int32)], [0, 1])))
    with pytest.raises(ValueError, match="leaves int32"):
        tstream.decode_embeds(tstream.read(hand_built([-top, np.full(P, -20, np.int32)], [0, 1])))


# ---------------------------------------------------------------------------------------------------------------------- surface
def test_flags_and_parser_errors(tmp_path):
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_compression as C
    p = C.build_parser()
    assert p.get_default("bitstream_temporal") is False
    assert p.parse_args(["--bitstream_temporal", "--bitstream_run", "256"]).bitstream_temporal is True
    with pytest.raises(SystemExit):
        C.main(["--bitstream", "x.bnrt", "--bitstream_temporal"])                             # N = 0: refused by the parser, before anything is built
    with pytest.raises(ValueError, match="HNeRV_Boost"):
        C.main(["--bitstream", "x.bnrt", "--bitstream_temporal", "--bitstream_run", "256", "--model", "NeRV_Boost", "--outf", str(tmp_path)])
    a = codec.build_parser().parse_args(["repack", "a", "b"])
    assert a.temporal is False and codec.build_parser().parse_args(["repack", "a", "b", "--temporal"]).temporal is True
    with pytest.raises(ValueError, match="wide=True"):
        codec.encode(None, None, None, None, io.BytesIO(), run=256, temporal=True)            # refused before the model is looked at
    with pytest.raises(ValueError, match="run > 0"):
        codec.encode(None, None, None, None, io.BytesIO(), wide=True, temporal=True)
    with pytest.raises(ValueError, match="wide=True"):
        codec.repack(b"BNRV", io.BytesIO(), 64, temporal=True)
    # the command line: --temporal implies the wide record; info tells the kind by its magic
    src, dst = str(tmp_path / "a.bnrv"), str(tmp_path / "a.bnrt")
    open(src, "wb").write(version1_blob(CASES["walk"]()))
    budget = codec.main(["repack", src, dst, "--run", "64", "--temporal"])
    assert budget["n_inter_frames"] == N_FRAMES - 1 and codec.main(["info", dst]) == budget
    assert open(dst, "rb").read() == _repacked("walk", 64, "gaussian")[0]


def test_header_declares_the_new_entry_points_and_the_abi_version_stays():
    import ctypes as C
    from boosting_nerv_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    assert int(re.search(r"#define\s+BNERV_CHAIN_UNROLL\s+(\d+)", header).group(1)) == _lib.CHAIN_UNROLL
    assert int(re.search(r"#define\s+BNERV_CHAIN_SEG\s+(\d+)", header).group(1)) == _lib.CHAIN_SEG
    assert C.sizeof(_lib.DeltaStats) == 24 and C.sizeof(_lib.RanswItem) == 48
    assert "ranst" in open(os.path.join(ROOT, "boosting_nerv_amd", "csrc", "build.sh")).read().split('UNITS="')[1].split('"')[0].split()
    lib = _lib.load()
    assert lib.bnerv_abi_version() == 9
    assert issubclass(ops.AnsDecodeWide, ops.AnsDequantWide)
    for cls in (ops.EmbedDelta, ops.AnsDecodeWide, ops.EmbedChainDequant):
        assert all(callable(getattr(cls, m)) for m in ("launch", "check"))
    # the launchers validate before they touch a device
    assert lib.bnerv_embed_delta(None, None, 0, 0, 0, None, 0, None) != 0
    assert lib.bnerv_rans_decode_wide(None, None, 0, None, 0, None, 0, None, 0, None, 0, 64, None) != 0
    assert b"rans_decode_wide" in lib.bnerv_last_error()
    assert lib.bnerv_embed_chain_dequant(None, None, 0, None, None, None, 0, 0, None, 0, None) != 0
    with pytest.raises(ValueError, match="no items"):
        ops.AnsDecodeWide(np.zeros(2, np.uint32), [], 64)
