"""The sparse post-hoc quantised model's file on the host: quant_tensor_sparse against quant_tensor and a numpy
restatement, the zero parse of the host coder against a pure-Python restatement, the host coder's refusals, the container, the parse
choice and the file sizes against the dense kind."""
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT
import qstream_cases as Q
import zstream_cases as Z

NEW_SYMBOLS = ("bnerv_huffz_encode", "bnerv_huffz_decode", "bnerv_huffz_dequant")
SETTINGS = {"model": "HNeRV", "fc_dim": 10, "enc_dim": "16_4", "final_size": 180 * 320, "full_data_length": 3, "crop_list": "180_320",
            "dec_strds": [5, 2, 2], "quant_model_bit": 8, "quant_embed_bit": 6, "huff_run": 256}
_cache = {}


def _five():
    if "five" not in _cache:
        _cache["five"] = Z.five_sparse_records(0.4)
    return _cache["five"]


# ---------------------------------------------------------------------------------------------------------------------- the twin
def test_quant_tensor_sparse_equals_quant_tensor_on_tensors_without_zeros():
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.hnerv_utils import quant_tensor, quant_tensor_sparse
    for t, want in zip(Q.five_tensors(), Q.FIVE_GEOMETRIES):
        assert bool((t != 0).all())
        dense, rebuilt_d = quant_tensor(t, 8)
        sparse, rebuilt_s = quant_tensor_sparse(t, 8)
        assert set(sparse) == set(dense) | {"keep"} and bool(sparse["keep"].all()) and sparse["keep"].shape == t.shape
        for k in dense:
            assert sparse[k].dtype == dense[k].dtype and sparse[k].shape == dense[k].shape and torch.equal(sparse[k], dense[k]), k
        assert torch.equal(rebuilt_s, rebuilt_d) and codec._grid_geometry(sparse) == want


@pytest.mark.parametrize("case", range(5))
def test_pruned_entries_stay_zero_and_the_rest_is_the_restatement(case):
    (q, keep, lo, step, outer, red, inner, flag), rebuilt, t = _five()[case]
    assert (outer, red, inner, flag) == Z.FIVE_SPARSE_GEOMETRIES[case]
    zeros = ~keep
    assert zeros.sum() == int(round(0.4 * q.size)) and np.array_equal(keep, t.reshape(-1).numpy() != 0)
    assert not rebuilt[zeros].any() and not np.signbit(rebuilt[zeros]).any() and not q[zeros].any()        # +0.0, code 0
    assert Z.restate(q, keep, lo, step, outer, red, inner).tobytes() == rebuilt.tobytes()
    assert np.array_equal(rebuilt[keep], Q.restate(q, lo, step, outer, red, inner)[keep])
    # the grid is fitted to the kept elements alone: no code is further than half a step (plus the fp16 rounding of the grid) from its value
    i = np.arange(q.size)
    s = (i // (red * inner)) * inner + i % inner
    assert np.all(np.abs(rebuilt - t.reshape(-1).numpy())[keep] <= 0.51 * step.astype(np.float32)[s][keep] + 2e-3 * np.abs(lo.astype(np.float32))[s][keep])


def test_all_zero_slices_one_value_slices_and_an_all_zero_tensor():
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.hnerv_utils import quant_tensor_sparse
    torch.manual_seed(5)
    t = torch.randn(60, 8, 3, 3)
    t[:, 3, 1, 1] = 0.0                                     # a slice of the winning grid without a kept element
    t[:, 5, 0, 2] = 0.0
    t[7, 5, 0, 2] = 0.37                                    # a slice with one kept value: step 0
    rec, rebuilt = quant_tensor_sparse(t, 8)
    assert codec._grid_geometry(rec) == (1, 60, 72, Z.F16)
    assert torch.isfinite(rebuilt).all() and all(torch.isfinite(rec[k].float()).all() for k in ("min", "scale"))
    half = torch.tensor(0.37).half().item()
    assert rec["min"][0, 3, 1, 1].item() == 0 and rec["scale"][0, 3, 1, 1].item() == 0 and rec["scale"][0, 5, 0, 2].item() == 0
    assert rec["min"][0, 5, 0, 2].item() == half and rebuilt[7, 5, 0, 2].item() == half
    assert not rebuilt[:, 3, 1, 1].any() and rebuilt[:, 5, 0, 2].count_nonzero() == 1 and not rec["quant"][:, 5, 0, 2].any()
    assert not rebuilt[t == 0].any() and torch.equal(rec["keep"], t != 0)      # (a kept value may still round to a grid point at 0.0)
    zero =torch.zeros(4, 5, 3)
    rec, rebuilt = quant_tensor_sparse(zero, 8)
    assert not rebuilt.any() and not rec["quant"].any() and not rec["keep"].any() and not rec["min"].any() and not rec["scale"].any()
    assert not torch.signbit(rebuilt).any()
    one = torch.full((7,), -2.5)                            # a constant tensor: step 0 on the per-tensor grid
    rec, rebuilt = quant_tensor_sparse(one, 8)
    assert torch.equal(rebuilt, one) and not rec["quant"].any() and rec["scale"].item() == 0


# ---------------------------------------------------------------------------------------------------------------------- the parse
def _kept(n, rng):
    return rng.integers(0, 256, size=n).astype(np.uint8)


def _parse_cases():
    """[(name, [host record, ...])]: stretches of 1, 2, 3, 255 and 256 zeros; a stretch across a run boundary; last runs of 1 and of 255
    elements; records of one element; zeros and kept elements alternating."""
    rng = np.random.default_rng(31)

    def rec(keep):
        keep = np.asarray(keep, dtype=bool)
        return Z.hand_record(keep.size, Z.F32, rng, keep, _kept(keep.size, rng))

    k = np.ones(4 * 256, dtype=bool)
    k[[1, 3, 4, 6, 7, 8]] = False                           # 1, 2 and 3 zeros between kept elements
    k[257:512] = False                                      # 255 zeros behind one kept element: to the end of run 1
    k[512:768] = False                                      # 256 zeros: all of run 2
    across = np.ones(600, dtype=bool)
    across[250:263] = False                                 # 13 zeros over the edge at 256: cut into 6 and 7
    return [("stretches", [rec(k)]), ("across", [rec(across)]), ("last_run_1", [rec(rng.random(257) < 0.5)]), ("last_run_255", [rec(rng.random(511) < 0.3)]),
            ("count_1", [rec([True]), rec([False]), rec([True])]), ("alternating", [rec(np.arange(700) % 2 == 0), rec(np.arange(300) % 2 == 1)]),
            ("all_zero", [rec(np.zeros(1000, dtype=bool))]), ("no_zero", [rec(np.ones(1000, dtype=bool))])]


def _python_decode(words, lengths, run_bits):
    """The leaves of every run, from the canonical code written out in plain Python: leaves by (length, index), first code 0, next = (code + 1)
    shifted left by the growth in length; bits most significant first."""
    table, code, prev = {}, 0, 0
    for ln, leaf in sorted((int(l), i) for i, l in enumerate(lengths) if l):
        code <<= ln - prev
        table[(ln, code)] = leaf
        code, prev = code + 1, ln
    bits = "".join(f"{int(w):032b}" for w in words)
    runs, pos = [], 0
    for nb in run_bits:
        end, leaves = pos + int(nb), []
        while pos < end:
            ln = 1
            while (ln, int(bits[pos:pos + ln], 2)) not in table:
                ln += 1
                assert ln <= 32
            leaves.append(table[(ln, int(bits[pos:pos + ln], 2))])
            pos += ln
        assert pos == end
        runs.append(leaves)
    return runs


@pytest.mark.parametrize("parse", Z.PARSES)
@pytest.mark.parametrize("name", [n for n, _ in _parse_cases()])
def test_host_coder_writes_the_restated_parse_and_decodes_it_back(name, parse):
    from boosting_nerv_amd import zstream
    from boosting_nerv_amd.lib.entropy_model import huffz_decode
    records = dict(_parse_cases())[name]
    words, lengths, split, used = Z.stream(records, parse)
    assert used == parse
    want = [leaves for r in records for leaves in Z.parse_leaves(r[0], r[1], parse)]
    got = _python_decode(words, lengths, np.concatenate(split))
    assert got == want
    assert all(len(leaves) <= 256 for leaves in want) and all(len(leaves) >= 1 for leaves in want)
    if name == "stretches":
        run1, run2 = want[1], want[2]
        assert run2 == ([Z.ZERO] * 256 if parse == "single" else [Z.ZERO + 8])
        assert run1[1:] == ([Z.ZERO] * 255 if parse == "single" else [Z.ZERO + k for k in range(7, -1, -1)])
        head = want[0][:10]
        zeros = [leaf for leaf in head if leaf >= Z.ZERO]
        assert zeros == ([Z.ZERO] * 6 if parse == "single" else [Z.ZERO, Z.ZERO + 1, Z.ZERO + 1, Z.ZERO])
    if name == "across" and parse == "runs":
        assert want[0][-2:] == [Z.ZERO + 2, Z.ZERO + 1] and want[1][:3] == [Z.ZERO + 2, Z.ZERO + 1, Z.ZERO]
    if name == "all_zero" and parse == "runs":
        assert want == [[Z.ZERO + 8]] * 3 + [[Z.ZERO + 7, Z.ZERO + 6, Z.ZERO + 5, Z.ZERO + 3]]
    symbols, keep, counts = np.concatenate([r[0] for r in records]), np.concatenate([r[1] for r in records]), [r[0].size for r in records]
    hist = np.bincount(np.concatenate([np.asarray(leaves, dtype=np.int64) for leaves in want]), minlength=Z.LEAVES - 1)
    assert np.array_equal(zstream.parse_histogram(symbols, keep, counts, parse), hist)
    assert int(np.concatenate(split).sum(dtype=np.int64)) == int((hist * lengths[:-1].astype(np.int64)).sum())
    sym, kp = huffz_decode(words, np.concatenate(split), counts, lengths)
    assert np.array_equal(sym, symbols) and np.array_equal(kp, keep) and kp.dtype == bool


def _hand_code(**lengths):
    ln = np.zeros(Z.LEAVES, dtype=np.uint8)
    for leaf, v in lengths.items():
        ln[int(leaf[1:])] = v
    return ln


def test_host_decoder_refuses_damaged_input():
    from boosting_nerv_amd._lib import BnervError
    from boosting_nerv_amd.lib.entropy_model import huffz_decode, huffz_encode
    rng = np.random.default_rng(32)
    rec = Z.hand_record(600, Z.F32, rng, 0.5)
    words, lengths, split, _ = Z.stream([rec])
    rb = split[0].copy()
    rb[0] += 1
    rb[1] -= 1                                              # the same total, another cut
    with pytest.raises(BnervError, match="does not end on its recorded bit|carries the run past"):
        huffz_decode(words, rb, [600], lengths)
    with pytest.raises(BnervError, match="add up"):         # the lengths do not add up to the words
        huffz_decode(words[:-1], split[0], [600], lengths)
    with pytest.raises(BnervError, match="runs"):
        huffz_decode(words, split[0][:-1], [600], lengths)
    # codes by hand: leaf 5 is `0`, a zero-run leaf `10`, EOF `11`
    code = _hand_code(l5=1, l258=2, l265=2)
    eof = np.array([0b110 << 29], dtype=np.uint32)          # EOF, then leaf 5
    with pytest.raises(BnervError, match="EOF"):
        huffz_decode(eof, np.array([3], dtype=np.uint16), [2], code)
    over = np.array([0b010 << 29], dtype=np.uint32)         # leaf 5, then four zeros in a run of three elements
    with pytest.raises(BnervError, match="carries the run past its 3 elements"):
        huffz_decode(over, np.array([3], dtype=np.uint16), [3], code)
    fits = huffz_decode(over, np.array([3], dtype=np.uint16), [5], code)
    assert fits[0].tolist() == [5, 0, 0, 0, 0] and fits[1].tolist() == [True, False, False, False, False]
    with pytest.raises(BnervError, match="Kraft"):
        huffz_decode(words, split[0], [600], np.ones(Z.LEAVES, dtype=np.uint8))
    with pytest.raises(BnervError, match="leaf 256 of item 0 has no code"):      # an encoder asked for a leaf the code lacks
        huffz_encode(np.array([5, 0], dtype=np.uint8), np.array([1, 0]), [2], _hand_code(l5=1, l265=1), "single")
    with pytest.raises(BnervError, match="R = 512"):
        huffz_encode(rec[0], rec[1], [600], lengths, "runs", run=512)


# ---------------------------------------------------------------------------------------------------------------------- container
def _file():
    if "blob" not in _cache:
        from boosting_nerv_amd import zstream
        records = [r for r, _, _ in _five()]
        words, lengths, split, parse = Z.stream(records)
        zrec = Z.zrecords(records, split)
        hist = Z.histogram(records, parse)
        settings = dict(SETTINGS, zero_parse=parse, n_zero_leaves=int(hist[Z.ZERO:].sum()))
        _cache.update(blob=zstream.to_bytes(settings, lengths, zrec, words), records=records, words=words, lengths=lengths, split=split, zrec=zrec,
                      settings=settings, hist=hist)
    return _cache["blob"], _cache


def _reframe(payload, magic=None):
    from boosting_nerv_amd import zstream
    return zstream._PREFIX.pack(magic or zstream.MAGIC, zstream.VERSION, len(payload)) + payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


def test_write_read_round_trip_and_budget(tmp_path):
    from boosting_nerv_amd import codec, zstream
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.lib.entropy_model import huffz_decode
    blob, c = _file()
    zs = zstream.read(io.BytesIO(blob))
    assert zs.settings == c["settings"] and np.array_equal(zs.lengths, c["lengths"]) and zs.lengths.dtype == np.uint8 and zs.lengths.size == 266
    assert np.array_equal(zs.words, c["words"]) and zs.words.dtype == np.uint32 and len(zs.records) == 5
    for got, rec, rb in zip(zs.records, c["records"], c["split"]):
        q, keep, lo, step, outer, red, inner, flag = rec
        assert (got.count, got.outer, got.red, got.inner, got.dtype, got.kept) == (q.size, outer, red, inner, flag, int(keep.sum()))
        assert got.min.tobytes() == lo.tobytes() and got.scale.tobytes() == step.tobytes() and np.array_equal(got.run_bits, rb)
    sym, keep = huffz_decode(zs.words, np.concatenate([r.run_bits for r in zs.records]), [r.count for r in zs.records], zs.lengths)
    at = 0
    for r, (rec, rebuilt, _) in zip(zs.records, _five()):
        assert Z.restate(sym[at:at + r.count], keep[at:at + r.count], r.min, r.scale, r.outer, r.red, r.inner).tobytes() == rebuilt.tobytes()
        assert int(keep[at:at + r.count].sum()) == r.kept
        at += r.count
    budget = zstream.info(blob)
    assert budget["total"] == 8 * len(blob) == sum(budget[k] for k in zstream.ITEMS) and budget["bytes"] == len(blob)
    hist = c["hist"]
    assert budget["symbol_bits"] == T._huffman_total_bits(hist[hist > 0].tolist()) == int((hist * c["lengths"][:-1].astype(np.int64)).sum())
    assert budget["code_table"] == 8 * 266 and budget["run_index"] == 16 * budget["n_runs"] and budget["padding"] < 32
    assert budget["n_zero_elements"] == sum(int((~r[1]).sum()) for r in c["records"]) and budget["n_symbols"] == sum(r[0].size for r in c["records"])
    assert budget["n_zero_leaves"] == int(hist[Z.ZERO:].sum()) and budget["zero_parse"] == c["settings"]["zero_parse"]
    path = tmp_path / "five.bnrz"
    assert zstream.write(str(path), c["settings"], c["lengths"], c["zrec"], c["words"]) == len(blob) and path.read_bytes() == blob
    assert zstream.info(str(path)) == budget == codec.info(str(path)) == codec.main(["info", str(path)])
    assert zstream.magic_of(str(path)) == b"BNRZ" and "zero-run leaves" in codec.describe_any(budget) and "Huffman codes" in codec.describe_sparse(budget)


def test_read_refusals():
    from boosting_nerv_amd import qstream, zstream
    blob, c = _file()
    with pytest.raises(ValueError, match="bad magic"):
        zstream.read(b"BNRQ" + blob[4:])
    with pytest.raises(ValueError, match="bad magic"):
        qstream.read(blob)                                  # and the dense reader does not take the sparse kind for its own
    with pytest.raises(ValueError, match="unknown format version"):
        zstream.read(blob[:4] + struct.pack("<I", zstream.VERSION + 1) + blob[8:])
    for cut in (0, 3, 15, 16, 40, len(blob) // 2, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated"):
            zstream.read(blob[:cut])
    for at in (20, len(blob) // 2, len(blob) - 6):
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(ValueError, match="CRC"):
            zstream.read(bytes(bad))
    payload = bytearray(blob[zstream._PREFIX.size:-4])
    n_header = struct.unpack_from("<I", payload)[0]
    table = 4 + n_header
    bad = bytearray(payload)
    used = int(np.flatnonzero(c["lengths"])[0])
    bad[table + used] += 1
    with pytest.raises(ValueError, match="Kraft"):
        zstream.read(_reframe(bytes(bad)))
    bad = bytearray(payload)
    bad[table + used] = 40
    with pytest.raises(ValueError, match="exceeds 32"):
        zstream.read(_reframe(bytes(bad)))
    rec0 = table + 266 + 4
    bad = bytearray(payload)
    struct.pack_into("<I", bad, rec0 + 20, 13)              # kept = 13 in a record of 12 elements
    with pytest.raises(ValueError, match="13 kept"):
        zstream.read(_reframe(bytes(bad)))
    bad = bytearray(payload)
    first_run = rec0 + 24 + 2 * 4                           # record 0: one fp32 pair, then its single run length
    struct.pack_into("<H", bad, first_run, struct.unpack_from("<H", bad, first_run)[0] + 64)
    with pytest.raises(ValueError, match="add up"):
        zstream.read(_reframe(bytes(bad)))
    with pytest.raises(ValueError, match="truncated"):      # a payload cut inside the bit string, re-framed with a good CRC
        zstream.read(_reframe(bytes(payload[:-8])))
    for key, value in (("zero_parse", "pairs"), ("n_zero_leaves", -1), ("n_zero_leaves", 0), ("huff_run", 512)):
        with pytest.raises(ValueError, match="zero|run length"):
            zstream.read(zstream.to_bytes(dict(c["settings"], **{key: value}), c["lengths"], c["zrec"], c["words"]))
    with pytest.raises(ValueError, match="zstream"):
        zstream.check_lengths(np.ones(266, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- parse choice and size
def _one_tensor_files(t, sparsity):
    """(BNRZ bytes, BNRQ bytes, zstream.info, qstream.info) of the one-tensor model `t` pruned to `sparsity`."""
    from boosting_nerv_amd import codec, qstream, zstream
    from boosting_nerv_amd.hnerv_utils import quant_tensor, quant_tensor_sparse
    p = Z.prune(t, sparsity)
    rec_s, _ = quant_tensor_sparse(p, 8)
    rec_d, _ = quant_tensor(p, 8)
    zr = Z.host_record(rec_s, codec._grid_geometry(rec_s))
    words, lengths, split, parse = Z.stream([zr])
    hist = zstream.parse_histogram(zr[0], zr[1], [zr[0].size], parse)
    z = zstream.to_bytes(dict(SETTINGS, zero_parse=parse, n_zero_leaves=int(hist[Z.ZERO:].sum())), lengths, Z.zrecords([zr], split), words)
    qr = Q.host_record(rec_d, codec._grid_geometry(rec_d))
    words, lengths, split = Q.stream([qr])
    q = qstream.to_bytes(SETTINGS, lengths, Q.qrecords([qr], split), words)
    return z, q, zstream.info(z), qstream.info(q), (zr, parse)


@pytest.mark.parametrize("sparsity", [0.4, 0.9])
def test_the_written_parse_is_the_one_with_fewer_bits(sparsity):
    """50 000 seeded Gaussian values on a per-tensor grid.  The condition is the minimum under both restatements (zstream.parse_histogram
    and the pure-Python parse); which parse that is -- the synthetic estimate of the issue says "single" at 0.4 and "runs" at 0.9 -- is
    printed, and asserted only through the minimum."""
    from boosting_nerv_amd import zstream
    from boosting_nerv_amd import train_nerv_all as T
    t = torch.randn(50000, generator=torch.Generator().manual_seed(40))
    z, _, budget, _, (zr, parse) = _one_tensor_files(t, sparsity)
    bits = {}
    for p in Z.PARSES:
        a, b = zstream.parse_histogram(zr[0], zr[1], [zr[0].size], p), Z.histogram([zr], p)
        assert np.array_equal(a, b)
        bits[p] = T._huffman_total_bits(a[a > 0].tolist())
    print(f"sparsity {sparsity}: {bits}, written {parse}: {budget['symbol_bits'] / 50000:.3f} bits per element")
    assert budget["zero_parse"] == parse == zstream.read(z).settings["zero_parse"]
    assert budget["symbol_bits"] == bits[parse] == min(bits.values())
    assert parse == "single" or bits["runs"] < bits["single"]          # "single" on a tie


@pytest.mark.parametrize("sparsity", [0.2, 0.4, 0.8])
def test_sparse_file_is_smaller_than_the_dense_file_of_the_same_pruned_tensor(sparsity):
    torch.manual_seed(0)
    t = torch.randn(96, 60, 3, 3) * 0.05
    z, q, bz, bq, (zr, _) = _one_tensor_files(t, sparsity)
    assert zr[4:] == (96, 60, 9, Z.F16)                     # a per-axis fp16 grid wins
    print(f"sparsity {sparsity}: BNRZ {len(z)} bytes ({bz['symbol_bits'] / zr[0].size:.3f} bits per element, {bz['zero_parse']}), BNRQ {len(q)} bytes "
          f"({bq['symbol_bits'] / zr[0].size:.3f})")
    assert len(z) < len(q)


def test_dense_tensor_costs_the_table_bytes_and_the_kept_counts_only():
    """At sparsity 0 the two kinds hold the same symbols under the same code: outside the JSON header the sparse file is larger by its 9 extra
    code lengths and 4 bytes of `kept` per record at most (the padding to a whole word is the same), and the header grows by exactly the two
    settings the format adds, zero_parse and n_zero_leaves."""
    import json
    torch.manual_seed(0)
    t = torch.randn(96, 60, 3, 3) * 0.05
    z, q, bz, bq, (zr, parse) = _one_tensor_files(t, 0.0)
    assert parse == "single" and bz["n_zero_elements"] == 0 == bz["n_zero_leaves"] and bz["symbol_bits"] == bq["symbol_bits"]
    assert bz["total"] - bz["header"] == bq["total"] - bq["header"] + 8 * (9 + 4 * 1)
    extra = len(json.dumps(dict(SETTINGS, zero_parse=parse, n_zero_leaves=0), sort_keys=True, separators=(",", ":"))) - \
        len(json.dumps(SETTINGS, sort_keys=True, separators=(",", ":")))
    assert bz["header"] - bq["header"] == 8 * extra and len(z) - len(q) == 9 + 4 + extra


# ---------------------------------------------------------------------------------------------------------------------- exports, CLI, model
def test_new_symbols_are_declared_bound_and_exported():
    from boosting_nerv_amd import _lib, ops, zstream
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    for macro, value in (("LEAVES", _lib.HUFFZ_LEAVES), ("ZERO", _lib.HUFFZ_ZERO), ("ZERO_LEAVES", _lib.HUFFZ_ZERO_LEAVES), ("SINGLE", _lib.HUFFZ_SINGLE),
                         ("RUNS", _lib.HUFFZ_RUNS)):
        assert int(re.search(r"#define\s+BNERV_HUFFZ_%s\s+(\d+)" % macro, header).group(1)) == value
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert callable(ops.huffz_dequant) and issubclass(ops.HuffzDequant, ops.HuffDequant)
    assert (zstream.LEAVES, zstream.ZERO, zstream.ZERO_LEAVES, zstream.RUN) == (_lib.HUFFZ_LEAVES, _lib.HUFFZ_ZERO, _lib.HUFFZ_ZERO_LEAVES, _lib.HUFF_RUN)
    assert zstream.PARSES.index("single") == _lib.HUFFZ_SINGLE and zstream.PARSES.index("runs") == _lib.HUFFZ_RUNS
    build = open(os.path.join(ROOT, "boosting_nerv_amd", "csrc", "build.sh")).read()
    assert "huffz.cpp" in build and re.search(r"UNITS=.*\bhuffz\b", build)


def test_dequant_entry_rejects_bad_arguments_before_touching_a_device():
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    _, c = _file()
    lengths = np.ascontiguousarray(c["lengths"])
    ln = lengths.ctypes.data
    a, odd = C.c_void_p(64), C.c_void_p(66)          # non-null addresses that are never dereferenced: every call below fails its checks first
    err = lambda: lib.bnerv_last_error()             # noqa: E731
    assert lib.bnerv_huffz_dequant(None, None, 8, a, 1, a, 1, ln, 256, a) == -1 and b"huffz_dequant" in err()
    assert lib.bnerv_huffz_dequant(None, a, 8, None, 1, a, 1, ln, 256, a) == -1
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, None, 1, ln, 256, a) == -1
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, a, 1, None, 256, a) == -1
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, a, 1, ln, 256, None) == -1
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, a, 1, ln, 128, a) == -1 and b"R = 128" in err()
    assert lib.bnerv_huffz_dequant(None, a, 2, a, 1, a, 1, ln, 256, a) == -1            # nothing but the padding
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 0, a, 1, ln, 256, a) == -1
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, a, 0, ln, 256, a) == -1
    assert lib.bnerv_huffz_dequant(None, odd, 8, a, 1, a, 1, ln, 256, a) == -1 and b"4-byte" in err()
    assert lib.bnerv_huffz_dequant(None, a, 8, C.c_void_p(68), 1, a, 1, ln, 256, a) == -1 and b"8-byte" in err()
    bad = lengths.copy()
    bad[np.flatnonzero(lengths)[0]] += 1             # an incomplete code
    assert lib.bnerv_huffz_dequant(None, a, 8, a, 1, a, 1, bad.ctypes.data, 256, a) == -1 and b"Kraft" in err()
    out = np.zeros(4, dtype=np.uint8)
    assert lib.bnerv_huffz_decode(None, 0, None, 0, None, 0, ln, 256, out.ctypes.data, out.ctypes.data) == -1 and b"huffz_decode" in err()
    assert lib.bnerv_huffz_encode(None, None, None, 0, ln, 0, 256, None, 0, None, 0) == -1 and b"huffz_encode" in err()


def test_flag_needs_a_file_and_repack_refuses_a_posthoc_file(tmp_path):
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    with pytest.raises(ValueError, match="--bitstream_sparse"):
        T.parse_args("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV -e 1 --bitstream_sparse".split())
    assert T.parse_args("--outf t -e 1 --bitstream f.bnrz --bitstream_sparse".split()).bitstream_sparse
    assert not T.parse_args("--outf t -e 1 --bitstream f.bnrq".split()).bitstream_sparse
    blob, _ = _file()
    with pytest.raises(NotImplementedError, match="no longer zero"):
        codec.repack(b"BNRQ" + blob[4:], io.BytesIO())
    with pytest.raises(NotImplementedError, match="--bitstream_sparse"):
        codec.repack(blob, str(tmp_path / "x.bnrc"))
    assert not os.path.exists(tmp_path / "x.bnrc")


def test_tiny_pruned_model_file_decodes_on_the_host_to_the_sparse_twin(tmp_path):
    """quant_model under --bitstream_sparse -> encode_posthoc -> zstream.read -> host decode -> restatement == the twin's state_dict, entry
    by entry; pruned weights are +0.0 in the twin; the report's bits are the file's symbol bits; the dense file of the same model is larger
    (CPU model, no kernel)."""
    from types import SimpleNamespace
    from oracle import configs
    from boosting_nerv_amd import codec, prune, zstream
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.lib.entropy_model import huffz_decode
    args = configs.tiny_nerv()
    args.__dict__.update(quant_model_bit=8, quant_embed_bit=6, crop_list="180_320", final_size=180 * 320, full_data_length=4, bitstream_sparse=True)
    torch.manual_seed(3)
    model = T.build_model(args)
    with torch.no_grad():
        flat = torch.cat([p.abs().flatten() for _, p in prune.prunable(model)])
        cut = flat.kthvalue(int(0.4 * flat.numel())).values
        for _, p in prune.prunable(model):
            p.mul_(p.abs() > cut)
    (_, twin), records = T.quant_model(model, args)
    prunable = {n for n, _ in prune.prunable(model)}
    assert {k for k, r in records.items() if "keep" in r} == {k for k, v in model.state_dict().items() if v.dim() > 1 and "encoder" not in k} >= prunable
    sd, src = twin.state_dict(), model.state_dict()
    for k in records:
        if "keep" in records[k]:
            assert torch.equal(sd[k] != 0, src[k] != 0) and not torch.signbit(sd[k][src[k] == 0]).any(), k
    path = str(tmp_path / "tiny.bnrz")
    budget = codec.encode_posthoc(model, args, records, None, path)
    lines = []
    T._huffman_report(args, records, None, SimpleNamespace(line=lines.append))
    assert budget == zstream.info(path) and budget["total"] == 8 * os.path.getsize(path)
    assert budget["symbol_bits"] == args.bits_per_param * budget["n_symbols"] and "bits per parameter" in lines[0]
    assert budget["n_zero_elements"] == sum(int((~r["keep"]).sum()) for r in records.values() if "keep" in r) > 0.3 * budget["n_symbols"]
    zs = zstream.read(path)
    assert zs.settings["model"] == "NeRV_Boost" and zs.settings["zero_parse"] in Z.PARSES and "bitstream_sparse" not in zs.settings
    sym, keep = huffz_decode(zs.words, np.concatenate([r.run_bits for r in zs.records]), [r.count for r in zs.records], zs.lengths)
    keys = [k for k in sd if "encoder" not in k]
    assert len(keys) == len(zs.records)
    at = 0
    for k, r in zip(keys, zs.records):
        got = Z.restate(sym[at:at + r.count], keep[at:at + r.count], r.min, r.scale, r.outer, r.red, r.inner)
        assert got.tobytes() == sd[k].reshape(-1).numpy().tobytes(), k
        at += r.count
    args.bitstream_sparse = False
    (_, _), dense = T.quant_model(model, args)
    assert not any("keep" in r for r in dense.values())
    dense_budget = codec.encode_posthoc(model, args, dense, None, io.BytesIO())
    print(f"tiny NeRV_Boost at 0.4: BNRZ {budget['bytes']} bytes, BNRQ {dense_budget['bytes']} bytes")
    assert "zero_parse" not in dense_budget and budget["bytes"] < dense_budget["bytes"]
