"""The chunked CEM file on the host: the runs coder of csrc/ans.cpp on the reference's own symbols, what cutting a
record into runs costs, the container and its refusals, damaged runs, codec.repack, and the C symbols.  No GPU: the host coder loads
without one."""
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

NEW_SYMBOLS = ("bnerv_ans_gaussian_cdf", "bnerv_ans_encode_gaussian_runs", "bnerv_ans_decode_gaussian_runs", "bnerv_rans_dequant")
SETTINGS = {"model": "NeRV_Boost", "fc_dim": 10, "full_data_length": 3, "crop_list": "180_320", "final_size": 180 * 320, "dec_strds": [5, 2, 2]}
RUNS = (64, 256, 1024)


def _golden():
    """[(name, int32 symbols, lo, hi, mean, std)]: what the REFERENCE's quantisers produced and the Gaussians its rate model fits."""
    npz = load_golden("cem.npz")
    out = []
    for name in ("w", "b"):
        sym = torch.from_numpy(npz[f"scale/{name}/quant"]).int().flatten().numpy()
        out.append((name, sym, int(sym.min()), int(sym.max()), float(npz[f"rate/{name}/mean"]), float(npz[f"rate/{name}/std"])))
    return out


def _spans(run_words):
    ends = np.cumsum(run_words.astype(np.int64))
    return list(zip(ends - run_words, ends))


def _round_trip(sym, lo, hi, mean, std, run):
    """encode in runs, decode all runs, decode every run on its own from its slice of the words -> (words, run_words)"""
    from boosting_nerv_amd.lib import entropy_model as em
    words, run_words = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, run)
    assert words.dtype == np.uint32 and run_words.dtype == np.uint16 and run_words.size == (sym.size + run - 1) // run
    assert int(run_words.sum()) == words.size and int(run_words.min()) >= 2
    assert np.array_equal(em.ans_decode_gaussian_runs(words, run_words, sym.size, lo, hi, mean, std, run), sym)
    for k, (a, b) in enumerate(_spans(run_words)):
        part = sym[k * run:(k + 1) * run]
        assert np.array_equal(em.ans_decode_gaussian_runs(words[a:b], run_words[k:k + 1], part.size, lo, hi, mean, std, run), part), k
    return words, run_words


# ---------------------------------------------------------------------------------------------------------------------- the coder
@pytest.mark.parametrize("run", RUNS)
def test_runs_round_trip_on_the_reference_symbols(run):
    for name, sym, lo, hi, mean, std in _golden():
        _round_trip(sym, lo, hi, mean, std, run)


def test_runs_round_trip_edge_cases():
    """A constant tensor (the support is widened to hi = lo + 1, as the encoder of the version-1 file does), a 3-symbol alphabet, and the
    counts around one run and one block of 64 runs, at run 64."""
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(11)
    words, run_words = _round_trip(np.full(300, 7, np.int32), 7, 8, 7.0, 1e-5, 64)
    assert np.array_equal(run_words, np.full(5, 2)) and not words.any()          # symbol 0 of every run from an empty state: the state stays empty
    _round_trip(np.full(300, 8, np.int32), 7, 8, 7.0, 1e-5, 64)                 # the other symbol costs the 24-bit leak each
    _round_trip(rng.integers(-1, 2, size=1000).astype(np.int32), -1, 1, 0.1, 0.7, 64)
    for n in (1, 63, 64, 65, 4097):
        sym = np.clip(np.rint(rng.normal(3.0, 11.0, size=n)), -40, 40).astype(np.int32)
        _, run_words = _round_trip(sym, -40, 40, 3.0, 11.0, 64)
        assert run_words.size == (n + 63) // 64
    # the table the three share
    cdf = em.ans_gaussian_cdf(-40, 40, 3.0, 11.0)
    assert cdf.dtype == np.uint32 and cdf.size == 82 and cdf[0] == 0 and cdf[-1] == 1 << 24 and (np.diff(cdf.astype(np.int64)) >= 1).all()
    from boosting_nerv_amd import _lib as L
    with pytest.raises(L.BnervError):
        em.ans_gaussian_cdf(3, 2, 0.0, 1.0)
    with pytest.raises(L.BnervError):
        em.ans_encode_gaussian_runs(np.array([9], np.int32), -4, 4, 0.0, 1.0, 64)
    with pytest.raises(L.BnervError):
        em.ans_encode_gaussian_runs(np.zeros(8, np.int32), -4, 4, 0.0, 1.0, 0)


def test_runs_equal_the_single_message_coder_run_by_run():
    """A run is a message of the existing coder: its words are ans_encode_gaussian's of the same symbols, the state padded to two words."""
    from boosting_nerv_amd.lib import entropy_model as em
    name, sym, lo, hi, mean, std = _golden()[0]
    words, run_words = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, 256)
    for k, (a, b) in list(enumerate(_spans(run_words)))[:40]:
        single = em.ans_encode_gaussian(sym[k * 256:(k + 1) * 256], lo, hi, mean, std)
        assert b - a - single.size in (0, 1, 2) and np.array_equal(words[a:a + single.size], single) and not words[a + single.size:b].any()


def test_cost_of_cutting_stays_within_the_per_message_bound():
    """For every run: bits <= ideal code length of the run's symbols under the record's Gaussian * 1.01 + 96 -- the per-message bound of
    tests/test_host_cpu.py (1 % + 64) plus 32 bits for the fixed second state word.  Prints the largest excess over the ideal length."""
    from boosting_nerv_amd.lib import entropy_model as em
    for name, sym, lo, hi, mean, std in _golden():
        n = torch.distributions.normal.Normal(torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64).clamp(1e-5, 1e10))
        z = n.cdf(torch.tensor(hi + 0.5, dtype=torch.float64)) - n.cdf(torch.tensor(lo - 0.5, dtype=torch.float64))
        q = torch.from_numpy(sym).double()
        bits = -torch.log2(((n.cdf(q + 0.5) - n.cdf(q - 0.5)) / z).clamp_min(1e-300)).numpy()      # em.ideal_code_bits, per symbol, on the record's support
        assert abs(bits.sum() - em.ideal_code_bits(torch.from_numpy(sym).float(), torch.tensor(mean), torch.tensor(std))) < 1e-6 * bits.sum()
        for run in RUNS:
            words, run_words = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, run)
            ideal = np.add.reduceat(bits, np.arange(0, sym.size, run))
            coded = 32.0 * run_words
            excess = coded - ideal
            k = int(excess.argmax())
            print(f"cem.npz {name} ({sym.size} symbols) run {run}: {run_words.size} runs, {coded.sum():.0f} bits against {bits.sum():.0f} ideal "
                  f"({coded.sum() / sym.size:.3f} against {bits.sum() / sym.size:.3f} per symbol); largest excess {excess[k]:.1f} bits in run {k} "
                  f"(bound 1% + 96: {0.01 * ideal[k] + 96:.1f})")
            assert (coded <= ideal * 1.01 + 96).all(), (name, run, k, coded[k], ideal[k])


def test_damaged_run_is_reported_and_reads_stay_inside_its_span():
    """One bit flipped in a bulk word of one run: the host runs-decoder names that run.  The same damaged run alone -- its own words and
    nothing around them -- fails the same way, and its neighbours, decoded on their own, are untouched: no decision depends on a word
    outside the span."""
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd.lib import entropy_model as em
    name, sym, lo, hi, mean, std = _golden()[0]
    sym = sym[:64 * 5]
    words, run_words = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, 64)
    spans = _spans(run_words)
    a, b = spans[2]
    assert b - a > 2                                      # run 2 has a bulk word
    bad = words.copy()
    bad[a] ^= 1 << 9
    with pytest.raises(L.BnervError, match=r"run 2 \("):
        em.ans_decode_gaussian_runs(bad, run_words, sym.size, lo, hi, mean, std, 64)
    with pytest.raises(L.BnervError, match=r"run 0 \("):
        em.ans_decode_gaussian_runs(bad[a:b], run_words[2:3], 64, lo, hi, mean, std, 64)
    for k in (1, 3):
        a2, b2 = spans[k]
        assert np.array_equal(em.ans_decode_gaussian_runs(bad[a2:b2], run_words[k:k + 1], 64, lo, hi, mean, std, 64), sym[64 * k:64 * k + 64])
    # a run cut short (one word moved to its neighbour: the counts still add up) fails in the run that lost the word
    moved = run_words.copy()
    moved[2] -= 1
    moved[3] += 1
    with pytest.raises(L.BnervError, match=r"run 2 \("):
        em.ans_decode_gaussian_runs(words, moved, sym.size, lo, hi, mean, std, 64)
    with pytest.raises(L.BnervError, match="add up"):
        em.ans_decode_gaussian_runs(words[:-1], run_words, sym.size, lo, hi, mean, std, 64)


# ---------------------------------------------------------------------------------------------------------------------- container
_cache = {}


def _file(run=64):
    if run not in _cache:
        from boosting_nerv_amd import rstream
        from boosting_nerv_amd.lib import entropy_model as em
        rng = np.random.default_rng(5)
        words, tensors, embeds, symbols = [], [], [], []

        def rec(sym, lo, hi, mean, std, beta=None):
            w, rw = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, run)
            words.append(w)
            symbols.append(sym)
            return rstream.RRecord(sym.size, np.float32(rng.uniform(0.01, 0.1)), np.float32(mean), np.float32(std), lo, hi, rw, beta)

        for name, sym, lo, hi, mean, std in _golden():
            tensors.append(rec(sym, lo, hi, float(np.float32(mean)), float(np.float32(std))))
        tensors.append(rec(np.full(12, -3, np.int32), -3, -2, -3.0, float(np.float32(1e-5))))
        for _ in range(3):
            sym = np.clip(np.rint(rng.normal(100.0, 30.0, size=2 * 4 * 5)), 0, 255).astype(np.int32)
            embeds.append(rec(sym, int(sym.min()), int(sym.max()), float(np.float32(sym.mean())), float(np.float32(sym.std())), np.float32(rng.normal())))
        raw = [rng.normal(size=7).astype(np.float32), rng.normal(size=1).astype(np.float32)]
        settings = dict(SETTINGS, ans_run=run)
        allw = np.concatenate(words)
        _cache[run] = dict(blob=rstream.to_bytes(settings, tensors, embeds, (2, 4, 5), raw, allw), settings=settings, tensors=tensors, embeds=embeds, raw=raw,
                           words=allw, symbols=symbols)
    return _cache[run]["blob"], _cache[run]


def _reframe(payload):
    from boosting_nerv_amd import rstream
    return rstream._PREFIX.pack(rstream.MAGIC, rstream.VERSION, len(payload)) + bytes(payload) + struct.pack("<I", zlib.crc32(bytes(payload)) & 0xFFFFFFFF)


def _payload(blob):
    from boosting_nerv_amd import rstream
    return bytearray(blob[rstream._PREFIX.size:-4])


def _same_record(got, want):
    assert (got.count, got.lo, got.hi) == (want.count, want.lo, want.hi)
    for f in ("scale", "mean", "std"):
        assert getattr(got, f).dtype == np.float32 and getattr(got, f) == getattr(want, f)
    assert np.array_equal(got.run_words, want.run_words) and got.run_words.dtype == np.uint16
    assert (got.beta is None) == (want.beta is None) and (want.beta is None or got.beta == want.beta)


@pytest.mark.parametrize("run", [64, 1024])
def test_write_read_gives_back_the_stream_and_the_budget_adds_up(tmp_path, run):
    from boosting_nerv_amd import rstream
    blob, c = _file(run)
    path = tmp_path / "x.bnrc"
    assert rstream.write(str(path), c["settings"], c["tensors"], c["embeds"], (2, 4, 5), c["raw"], c["words"]) == len(blob)
    assert path.read_bytes() == blob and blob[:4] == b"BNRC"
    for src in (blob, io.BytesIO(blob), str(path)):
        rs = rstream.read(src)
        assert rs.settings == c["settings"] and rs.embed_shape == (2, 4, 5)
        assert np.array_equal(rs.words, c["words"]) and rs.words.dtype == np.uint32
        assert len(rs.tensors) == 3 and len(rs.embeds) == 3
        for got, want in zip(rs.tensors + rs.embeds, c["tensors"] + c["embeds"]):
            _same_record(got, want)
        assert len(rs.raw) == 2 and all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(rs.raw, c["raw"]))
    for k, sym in enumerate(c["symbols"]):
        assert np.array_equal(rstream.decode_record(rs, k), sym), k
    b = rstream.info(blob)
    n_runs = sum(r.run_words.size for r in c["tensors"] + c["embeds"])
    assert sum(b[k] for k in rstream.ITEMS) == b["total"] == 8 * len(blob) and b["bytes"] == len(blob)
    assert b["ans_words"] == 32 * c["words"].size and b["run_index"] == 16 * n_runs == 16 * b["n_runs"] and b["padding"] == 64
    assert b["tensor_side"] == 3 * 24 * 8 and b["embed_side"] == 3 * 28 * 8 and b["raw"] == 8 * (4 * 8 + 2 * 4)
    assert (b["n_tensors"], b["n_embeds"], b["n_raw"], b["ans_run"]) == (3, 3, 2, run) and b["n_symbols"] == sum(s.size for s in c["symbols"])


def test_read_refusals():
    from boosting_nerv_amd import bitstream, rstream
    blob, c = _file(64)
    with pytest.raises(ValueError, match="magic"):
        rstream.read(b"BNRV" + blob[4:])
    with pytest.raises(ValueError, match="magic"):
        bitstream.read(blob)                              # and the version-1 reader refuses the new kind
    with pytest.raises(ValueError, match="version"):
        rstream.read(blob[:4] + struct.pack("<I", 2) + blob[8:])
    for cut in (3, 15, len(blob) // 2, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated"):
            rstream.read(blob[:cut])
    flipped = bytearray(blob)
    flipped[len(blob) // 2] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        rstream.read(bytes(flipped))
    # the remaining refusals are about the payload: edit bytes, recompute the CRC
    p = _payload(blob)
    n_header = struct.unpack_from("<I", p, 0)[0]
    rec0 = 4 + n_header + 4                               # the first record
    count0 = struct.unpack_from("<I", p, rec0)[0]
    runs0 = (count0 + 63) // 64
    q = bytearray(p)
    w = struct.unpack_from("<H", q, rec0 + 24)[0]
    struct.pack_into("<H", q, rec0 + 24, w + 1)           # one run claims a word more than the payload has
    with pytest.raises(ValueError, match="add up"):
        rstream.read(_reframe(q))
    q = bytearray(p)
    w0, w1 = struct.unpack_from("<HH", q, rec0 + 24)
    struct.pack_into("<HH", q, rec0 + 24, 1, w0 + w1 - 1)  # the sum holds, but a run is shorter than its state
    with pytest.raises(ValueError, match="two state words"):
        rstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<ii", q, rec0 + 16, -2048, 2048)    # 4097 symbols
    with pytest.raises(ValueError, match="alphabet"):
        rstream.read(_reframe(q))
    q = bytearray(p)
    struct.pack_into("<ii", q, rec0 + 16, -2048, 2047)    # 4096 are read
    rstream.read(_reframe(q))
    q = bytearray(p)
    q[-1] = 1                                             # the padding
    with pytest.raises(ValueError, match="not zero"):
        rstream.read(_reframe(q))
    with pytest.raises(ValueError, match="follow"):
        rstream.read(_reframe(p + b"\0\0\0\0"))
    assert runs0 > 1
    for bad in (0, 32, 96, 100, 4160, 8192, "64", None, 64.0):
        s = dict(c["settings"], ans_run=bad)
        header = __import__("json").dumps(s, sort_keys=True, separators=(",", ":")).encode()
        with pytest.raises(ValueError, match="run length"):
            rstream.read(_reframe(struct.pack("<I", len(header)) + header + bytes(p[4 + n_header:])))
        with pytest.raises(ValueError, match="run length"):
            rstream.to_bytes(s, c["tensors"], c["embeds"], (2, 4, 5), c["raw"], c["words"])


# ---------------------------------------------------------------------------------------------------------------------- repack
def _version1_blob():
    """A hand-built version-1 file: records from the golden symbols (and three small embedding records), coded as codec.encode codes them."""
    from boosting_nerv_amd import bitstream
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(9)
    symbols, tensors, embeds = [], [], []
    for name, sym, lo, hi, mean, std in _golden():
        mean, std = float(np.float32(mean)), float(np.float32(std))
        tensors.append(bitstream.Record(sym.size, np.float32(0.037), np.float32(mean), np.float32(std), lo, hi, em.ans_encode_gaussian(sym, lo, hi, mean, std)))
        symbols.append(sym)
    for _ in range(3):
        sym = np.clip(np.rint(rng.normal(100.0, 30.0, size=40)), 0, 255).astype(np.int32)
        lo, hi, mean, std = int(sym.min()), int(sym.max()), float(np.float32(sym.mean())), float(np.float32(sym.std()))
        embeds.append(bitstream.Record(40, np.float32(0.5), np.float32(mean), np.float32(std), lo, hi, em.ans_encode_gaussian(sym, lo, hi, mean, std), np.float32(rng.normal())))
        symbols.append(sym)
    raw = [rng.normal(size=9).astype(np.float32), rng.normal(size=2).astype(np.float32)]
    return bitstream.to_bytes(dict(SETTINGS, model="HNeRV_Boost"), tensors, embeds, (2, 4, 5), raw), symbols


@pytest.mark.parametrize("run", [64, 1024])
def test_repack_keeps_settings_side_values_raw_section_and_symbols(tmp_path, run):
    from boosting_nerv_amd import bitstream, codec, rstream
    blob, symbols = _version1_blob()
    src = bitstream.read(blob)
    out = io.BytesIO()
    budget = codec.repack(blob, out, run)
    assert budget == rstream.info(out.getvalue()) == codec.info(out.getvalue()) and budget["total"] == 8 * len(out.getvalue())
    assert "ANS words" in codec.describe_any(budget) and "coded words" in codec.describe_any(bitstream.info(blob))
    rs = rstream.read(out.getvalue())
    assert rs.settings == dict(src.settings, ans_run=run) and rs.embed_shape == src.embed_shape
    assert len(rs.raw) == len(src.raw) and all(np.array_equal(a, b) for a, b in zip(rs.raw, src.raw))
    for k, (got, want) in enumerate(zip(rs.tensors + rs.embeds, src.tensors + src.embeds)):
        assert (got.count, got.lo, got.hi) == (want.count, want.lo, want.hi)
        assert all(getattr(got, f).tobytes() == getattr(want, f).tobytes() for f in ("scale", "mean", "std"))
        assert (got.beta is None) == (want.beta is None) and (want.beta is None or got.beta.tobytes() == want.beta.tobytes())
        assert np.array_equal(rstream.decode_record(rs, k), symbols[k]), k
    # files by name and the command line; the default run
    a, b = tmp_path / "in.bnrv", tmp_path / "out.bnrc"
    a.write_bytes(blob)
    assert codec.main(["repack", str(a), str(b), "--run", str(run)]) == budget and b.read_bytes() == out.getvalue()
    assert codec.main(["info", str(b)]) == budget
    assert codec.repack(str(a), str(b))["ans_run"] == 1024
    with pytest.raises(ValueError, match="run length"):
        codec.repack(blob, io.BytesIO(), 100)
    with pytest.raises(ValueError, match="magic"):
        codec.repack(out.getvalue(), io.BytesIO(), run)   # only a version-1 file is a source


# ---------------------------------------------------------------------------------------------------------------------- C surface
def test_header_declares_the_new_entry_points_and_the_abi_version_stays():
    import ctypes as C
    from boosting_nerv_amd import _lib, ops, rstream
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    for macro, value in (("MAX_ALPHABET", _lib.RANS_MAX_ALPHABET), ("MIN_RUN", _lib.RANS_MIN_RUN), ("MAX_RUN", _lib.RANS_MAX_RUN)):
        assert int(re.search(r"#define\s+BNERV_RANS_%s\s+(\d+)" % macro, header).group(1)) == value
    assert (rstream.MAX_ALPHABET, rstream.MIN_RUN, rstream.MAX_RUN) == (_lib.RANS_MAX_ALPHABET, _lib.RANS_MIN_RUN, _lib.RANS_MAX_RUN)
    assert C.sizeof(_lib.RansBlock) == 16 and C.sizeof(_lib.RansItem) == 40
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.bnerv_abi_version() == 9
    assert callable(ops.ans_dequant)
    # the launcher validates before it touches a device
    assert lib.bnerv_rans_dequant(None, None, 0, None, 0, None, 0, None, 0, None, 0, 64, None) != 0
    assert b"null" in lib.bnerv_last_error()
