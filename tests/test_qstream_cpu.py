"""The post-hoc quantised model's file on the host: the container, the code lengths against the Huffman accounting of
train_nerv_all, the host coder of the library, the C symbols, and a numpy restatement of the de-quantisation against quant_tensor."""
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import ROOT
import qstream_cases as Q

NEW_SYMBOLS = ("bnerv_huff_encode", "bnerv_huff_decode", "bnerv_huff_dequant")
SETTINGS = {"model": "HNeRV", "fc_dim": 10, "enc_dim": "16_4", "final_size": 180 * 320, "full_data_length": 3, "crop_list": "180_320",
            "dec_strds": [5, 2, 2], "quant_model_bit": 8, "quant_embed_bit": 6, "huff_run": 256}


def _records():
    rng = np.random.default_rng(7)
    gauss = lambda n: np.rint(rng.normal(128, 20, size=n)).clip(0, 255).astype(np.uint8)      # noqa: E731
    return [Q.hand_record((3, 5, 7), Q.F16, rng, gauss(105)), Q.hand_record(1, Q.F32, rng, gauss(1)), Q.hand_record(256, Q.F32, rng, gauss(256)),
            Q.hand_record((1, 257, 3), Q.F16, rng, gauss(771)), Q.hand_record(70001, Q.F32, rng, gauss(70001))]


_cache = {}


def _file():
    if not _cache:
        from boosting_nerv_amd import qstream
        records = _records()
        words, lengths, split = Q.stream(records)
        qrec = Q.qrecords(records, split)
        _cache.update(blob=qstream.to_bytes(SETTINGS, lengths, qrec, words), records=records, words=words, lengths=lengths, split=split, qrec=qrec)
    return _cache["blob"], _cache


def _reframe(payload):
    from boosting_nerv_amd import qstream
    return qstream._PREFIX.pack(qstream.MAGIC, qstream.VERSION, len(payload)) + payload + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF)


def _payload(blob):
    from boosting_nerv_amd import qstream
    return bytearray(blob[qstream._PREFIX.size:-4])


# ---------------------------------------------------------------------------------------------------------------------- container
def test_round_trip_fields_symbols_and_budget(tmp_path):
    from boosting_nerv_amd import qstream
    from boosting_nerv_amd.lib.entropy_model import huff_decode
    blob, c = _file()
    qs = qstream.read(io.BytesIO(blob))
    assert qs.settings == SETTINGS and np.array_equal(qs.lengths, c["lengths"]) and qs.lengths.dtype == np.uint8
    assert np.array_equal(qs.words, c["words"]) and qs.words.dtype == np.uint32 and len(qs.records) == 5
    for got, rec, rb in zip(qs.records, c["records"], c["split"]):
        q, lo, step, outer, red, inner, flag = rec
        assert (got.count, got.outer, got.red, got.inner, got.dtype) == (q.size, outer, red, inner, flag)
        assert got.min.dtype == lo.dtype and got.min.tobytes() == lo.tobytes() and got.scale.tobytes() == step.tobytes()      # bit-equal, fp16 kept fp16
        assert np.array_equal(got.run_bits, rb)
    sym = huff_decode(qs.words, np.concatenate([r.run_bits for r in qs.records]), [r.count for r in qs.records], qs.lengths)
    assert np.array_equal(sym, np.concatenate([r[0] for r in c["records"]]))
    budget = qstream.info(blob)
    assert budget["total"] == 8 * len(blob) == sum(budget[k] for k in qstream.ITEMS) and budget["bytes"] == len(blob)
    all_sym = np.concatenate([r[0] for r in c["records"]])
    assert budget["symbol_bits"] == int(c["lengths"][all_sym].astype(np.int64).sum())
    n_runs = sum(rb.size for rb in c["split"])
    assert budget["run_index"] == 16 * n_runs == 16 * sum((r[0].size + 255) // 256 for r in c["records"]) and budget["n_runs"] == n_runs
    assert budget["code_table"] == 8 * 257 and budget["padding"] == 32 * c["words"].size - budget["symbol_bits"] and 0 <= budget["padding"] < 32
    assert budget["grid_side"] == sum(5 * 32 + 2 * r[1].size * r[1].itemsize * 8 for r in c["records"])
    assert budget["n_records"] == 5 and budget["n_symbols"] == all_sym.size
    # file and buffer forms agree
    path = tmp_path / "m.bnrq"
    assert qstream.write(str(path), SETTINGS, c["lengths"], c["qrec"], c["words"]) == len(blob) and path.read_bytes() == blob
    assert qstream.info(str(path)) == budget == qstream.info(io.BytesIO(blob))
    assert qstream.magic_of(str(path)) == qstream.magic_of(blob) == qstream.magic_of(io.BytesIO(blob)) == b"BNRQ"


def test_rejects_bad_magic_and_bumped_version_and_bitstream_read_answers_magic():
    from boosting_nerv_amd import bitstream, qstream
    blob, _ = _file()
    with pytest.raises(ValueError, match="magic"):
        qstream.read(b"BNRV" + blob[4:])
    bumped = blob[:4] + struct.pack("<I", qstream.VERSION + 1) + blob[8:]
    with pytest.raises(ValueError, match="version"):
        qstream.read(bumped)
    with pytest.raises(ValueError, match="version"):
        qstream.info(bumped)
    with pytest.raises(ValueError, match="magic"):
        bitstream.read(blob)


@pytest.mark.parametrize("where", ["prefix", "middle", "last_byte"])
def test_rejects_truncated_file(where):
    from boosting_nerv_amd import qstream
    blob, _ = _file()
    cut = {"prefix": 9, "middle": len(blob) // 2, "last_byte": len(blob) - 1}[where]
    with pytest.raises(ValueError, match="truncated"):
        qstream.read(blob[:cut])
    with pytest.raises(ValueError, match="truncated"):
        qstream.read(io.BytesIO(blob[:cut]))


def test_rejects_flipped_payload_byte():
    from boosting_nerv_amd import qstream
    blob, _ = _file()
    for pos in (16, len(blob) // 2, len(blob) - 5):
        bad = bytearray(blob)
        bad[pos] ^= 0x10
        with pytest.raises(ValueError, match="CRC"):
            qstream.read(bytes(bad))


def test_rejects_kraft_violation_long_code_and_run_lengths_that_do_not_sum():
    """Damage behind a valid CRC: the payload is edited and re-framed."""
    from boosting_nerv_amd import qstream
    blob, c = _file()
    p = _payload(blob)
    n_header, = struct.unpack_from("<I", p, 0)
    table = 4 + n_header
    assert bytes(p[table:table + 257]) == c["lengths"].tobytes()
    used = int(np.flatnonzero(c["lengths"])[0])
    bad = bytearray(p)
    bad[table + used] += 1                                  # one leaf a bit deeper: the Kraft sum falls below 1
    with pytest.raises(ValueError, match="Kraft"):
        qstream.read(_reframe(bytes(bad)))
    bad = bytearray(p)
    bad[table + 256] = 0                                    # no EOF leaf
    with pytest.raises(ValueError, match="Kraft"):
        qstream.read(_reframe(bytes(bad)))
    bad = bytearray(p)
    bad[table + used] = 33
    with pytest.raises(ValueError, match="exceeds 32"):
        qstream.read(_reframe(bytes(bad)))
    # first record: 20 bytes of fields, 2 x 21 fp16 grid entries, then its single u16 run length
    at = table + 257 + 4 + 20 + 2 * 21 * 2
    assert struct.unpack_from("<H", p, at)[0] == int(c["split"][0][0])
    bad = bytearray(p)
    struct.pack_into("<H", bad, at, int(c["split"][0][0]) + 40)
    with pytest.raises(ValueError, match="add up"):
        qstream.read(_reframe(bytes(bad)))
    with pytest.raises(ValueError, match="Kraft"):
        qstream.check_lengths(np.ones(257, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- code lengths
def _lengths_total(hist):
    """symbol_bits a file would book for a histogram over symbols 0..255: sum of count * code length."""
    from boosting_nerv_amd import codec
    lengths = codec.huffman_lengths(hist)
    return lengths, int((np.asarray(hist, dtype=np.int64) * lengths[:256].astype(np.int64)).sum())


def test_depths_reproduce_huffman_total_bits_on_random_histograms():
    from boosting_nerv_amd import qstream
    from boosting_nerv_amd.train_nerv_all import _huffman_depths, _huffman_total_bits
    rng = np.random.default_rng(3)
    for trial in range(12):
        hist = np.zeros(256, dtype=np.int64)
        k = int(rng.integers(2, 257))
        where = rng.choice(256, size=k, replace=False)
        hist[where] = rng.integers(1, 10 ** int(rng.integers(1, 6)), size=k)
        lengths, total = _lengths_total(hist)
        counts = hist[hist > 0].tolist()
        assert total == _huffman_total_bits(counts), trial
        depths = _huffman_depths(counts)
        assert len(depths) == len(counts) + 1 and lengths[256] == depths[-1] and np.array_equal(lengths[:256][hist > 0], depths[:-1])
        assert not lengths[:256][hist == 0].any()
        qstream.check_lengths(lengths)                      # a Huffman tree is complete: Kraft equality


def test_depths_on_a_one_symbol_alphabet():
    from boosting_nerv_amd.train_nerv_all import _huffman_depths, _huffman_total_bits
    hist = np.zeros(256, dtype=np.int64)
    hist[7] = 300
    lengths, total = _lengths_total(hist)
    assert _huffman_depths([300]) == [1, 1] and lengths[7] == 1 and lengths[256] == 1 and lengths.sum() == 2      # the EOF leaf is the sibling
    assert total == 300 == _huffman_total_bits([300])


def test_depths_on_the_power_of_two_histogram_reach_16():
    from boosting_nerv_amd.train_nerv_all import _huffman_depths, _huffman_total_bits
    counts = [2 ** k for k in range(16)]
    assert sum(counts) == 65535
    depths = _huffman_depths(counts)
    assert max(depths) == 16 and depths[0] == 16 and depths[-1] == 16 and depths[15] == 1
    sym = Q.depth16_symbols()
    lengths, total = _lengths_total(np.bincount(sym, minlength=256))
    assert total == _huffman_total_bits(counts) == sum(c * d for c, d in zip(counts, depths)) and lengths.max() == 16


def test_huffman_total_bits_keeps_its_values():
    from boosting_nerv_amd.train_nerv_all import _huffman_total_bits
    """Values the function returned before it was split into depths and a sum."""
    assert _huffman_total_bits([5, 9, 12, 13, 16, 45]) == 229          # (224 for the textbook six-symbol code; the EOF leaf deepens the rarest)
    assert _huffman_total_bits([1]) == 1 and _huffman_total_bits([1, 1]) == 4 and _huffman_total_bits([10, 10, 10, 10]) == 90
    assert _huffman_total_bits([3, 1, 4, 1, 5, 9, 2, 6]) == 87 and _huffman_total_bits([300]) == 300
    assert _huffman_total_bits([2 ** k for k in range(16)]) == 131054
    assert _huffman_total_bits([]) == 0


def test_a_code_deeper_than_32_is_refused_not_limited():
    from boosting_nerv_amd import codec
    hist = np.zeros(256, dtype=np.int64)
    hist[:40] = [2 ** k for k in range(40)]                 # depth 40 under this construction
    with pytest.raises(NotImplementedError, match="32"):
        codec.huffman_lengths(hist)


# ---------------------------------------------------------------------------------------------------------------------- host coder
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 256 + 5])
def test_host_coder_round_trip(n):
    from boosting_nerv_amd.lib.entropy_model import huff_decode
    rng = np.random.default_rng(n)
    records = [Q.hand_record(n, Q.F32, rng), Q.hand_record(3, Q.F32, rng)]          # a second item: the run after a short last run
    words, lengths, split = Q.stream(records)
    assert [rb.size for rb in split] == [(n + 255) // 256, 1]
    sym = np.concatenate([r[0] for r in records])
    bits = lengths[sym].astype(np.int64)
    assert int(split[0].sum()) == int(bits[:n].sum()) and int(split[1].sum()) == int(bits[n:].sum())
    assert words.size == (int(bits.sum()) + 31) // 32
    got = huff_decode(words, np.concatenate(split), [n, 3], lengths)
    assert got.dtype == np.uint8 and np.array_equal(got, sym)


def test_host_coder_bit_order_and_canonical_codes():
    """Lengths {a: 1, b: 2, EOF: 2}: canonical codes a = 0, b = 10, EOF = 11; "abba" = 0 10 10 0, most significant bit first."""
    from boosting_nerv_amd.lib.entropy_model import huff_encode
    lengths = np.zeros(257, dtype=np.uint8)
    lengths[[10, 20, 256]] = (1, 2, 2)
    words, run_bits = huff_encode(np.array([10, 20, 20, 10], dtype=np.uint8), [4], lengths)
    assert run_bits.tolist() == [6] and words.tolist() == [0b010100 << 26]


def test_host_decode_reports_a_wrong_run_length_and_a_missing_code():
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd.lib.entropy_model import huff_decode, huff_encode
    rng = np.random.default_rng(5)
    records = [Q.hand_record(600, Q.F32, rng)]
    words, lengths, split = Q.stream(records)
    rb = split[0].copy()
    rb[0] += 1
    rb[1] -= 1                                              # the total still matches the words: only the run boundary is wrong
    with pytest.raises(L.BnervError, match="recorded bit"):
        huff_decode(words, rb, [600], lengths)
    rb = split[0].copy()
    rb[2] += 64
    with pytest.raises(L.BnervError, match="add up"):
        huff_decode(words, rb, [600], lengths)
    with pytest.raises(L.BnervError, match="Kraft"):
        huff_decode(words, split[0], [600], np.ones(257, dtype=np.uint8))
    hole = np.zeros(257, dtype=np.uint8)
    hole[[1, 256]] = 1
    with pytest.raises(L.BnervError, match="no code"):
        huff_encode(np.array([1, 2], dtype=np.uint8), [2], hole)


# ---------------------------------------------------------------------------------------------------------------------- exports
def test_new_symbols_are_declared_bound_and_exported():
    import ctypes as C
    from boosting_nerv_amd import _lib
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    for macro, value in (("RUN", _lib.HUFF_RUN), ("LEAVES", _lib.HUFF_LEAVES), ("LUT_BITS", _lib.HUFF_LUT_BITS), ("F16", _lib.HUFF_F16)):
        assert int(re.search(r"#define\s+BNERV_HUFF_%s\s+(\d+)" % macro, header).group(1)) == value
    assert C.sizeof(_lib.HuffRun) == 16 and C.sizeof(_lib.HuffItem) == 40
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.bnerv_abi_version() == 9
    from boosting_nerv_amd import ops, qstream
    assert callable(ops.huff_dequant) and qstream.RUN == _lib.HUFF_RUN and qstream.LEAVES == _lib.HUFF_LEAVES
    assert "huff" in open(os.path.join(ROOT, "boosting_nerv_amd", "csrc", "build.sh")).read()


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    _, c = _file()
    lengths = np.ascontiguousarray(c["lengths"])
    ln = lengths.ctypes.data
    a, odd = C.c_void_p(64), C.c_void_p(66)          # non-null addresses that are never dereferenced: every call below fails its checks first
    err = lambda: lib.bnerv_last_error()             # noqa: E731
    assert lib.bnerv_huff_dequant(None, None, 8, a, 1, a, 1, ln, 256, a) == -1 and b"huff_dequant" in err()
    assert lib.bnerv_huff_dequant(None, a, 8, None, 1, a, 1, ln, 256, a) == -1
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, None, 1, ln, 256, a) == -1
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, None, 256, a) == -1
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, ln, 256, None) == -1
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, ln, 128, a) == -1 and b"R = 128" in err()
    assert lib.bnerv_huff_dequant(None, a, 2, a, 1, a, 1, ln, 256, a) == -1            # nothing but the padding
    assert lib.bnerv_huff_dequant(None, a, 8, a, 0, a, 1, ln, 256, a) == -1
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 0, ln, 256, a) == -1
    assert lib.bnerv_huff_dequant(None, odd, 8, a, 1, a, 1, ln, 256, a) == -1 and b"4-byte" in err()
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, ln, 256, odd) == -1 and b"4-byte" in err()
    assert lib.bnerv_huff_dequant(None, a, 8, C.c_void_p(68), 1, a, 1, ln, 256, a) == -1 and b"8-byte" in err()
    bad = np.ones(257, dtype=np.uint8)
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, bad.ctypes.data, 256, a) == -1 and b"Kraft" in err()
    bad = lengths.copy()
    bad[np.flatnonzero(lengths)[0]] = 40
    assert lib.bnerv_huff_dequant(None, a, 8, a, 1, a, 1, bad.ctypes.data, 256, a) == -1 and b"exceeds 32" in err()
    out = np.zeros(4, dtype=np.uint8)
    assert lib.bnerv_huff_decode(None, 0, None, 0, None, 0, ln, 256, out.ctypes.data) == -1 and b"huff_decode" in err()
    assert lib.bnerv_huff_encode(None, None, 0, ln, 256, None, 0, None, 0) == -1 and b"huff_encode" in err()


def test_encode_posthoc_refuses_what_no_file_can_hold():
    import torch
    from types import SimpleNamespace
    from boosting_nerv_amd import codec
    m = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match="quant_model_bit -1"):
        codec.encode_posthoc(m, SimpleNamespace(model="NeRV_Boost", quant_model_bit=-1), None, None, io.BytesIO())
    with pytest.raises(NotImplementedError, match="embed_inter"):
        codec.encode_posthoc(m, SimpleNamespace(model="HNeRV", quant_model_bit=8, interpolation=True, embed_inter=True), {}, None, io.BytesIO())
    with pytest.raises(NotImplementedError, match="no bitstream"):
        codec.encode_posthoc(m, SimpleNamespace(model="Other", quant_model_bit=8), {}, None, io.BytesIO())


def test_train_script_refuses_the_flags_before_it_trains(tmp_path, monkeypatch):
    """--bitstream with flags no file can serve stops right after argument parsing: no output directory, no device, no epoch."""
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    base = "--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV --crop_list 180_320 -e 1 --bitstream f.bnrq"
    with pytest.raises(NotImplementedError, match="quant_model_bit -1"):
        T.main((base + " --quant_model_bit -1").split())
    with pytest.raises(NotImplementedError, match="embed_inter"):
        T.main((base + " --interpolation --embed_inter").split())
    assert not os.path.exists(tmp_path / "output") and not os.path.exists(tmp_path / "f.bnrq")


# ---------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", range(5))
def test_numpy_restatement_equals_quant_tensor_rebuilt(case):
    """fp32(min) + fp32(scale) * fp32(q), two roundings, IS `rebuilt` -- and hnerv_utils.dequant_tensor is not, for fp16 grids."""
    (q, lo, step, outer, red, inner, flag), rebuilt = _five()[case]
    assert (outer, red, inner, flag) == Q.FIVE_GEOMETRIES[case]
    assert lo.dtype == (np.float16 if flag == Q.F16 else np.float32) and lo.size == outer * inner == step.size and q.size == outer * red * inner
    got = Q.restate(q, lo, step, outer, red, inner)
    assert got.dtype == np.float32 and got.tobytes() == rebuilt.tobytes()


def _five():
    if "five" not in _cache:
        _cache["five"] = Q.five_records()
    return _cache["five"]


def test_tiny_model_file_decodes_on_the_host_to_the_twin(tmp_path):
    """quant_model -> encode_posthoc -> qstream.read -> host decode -> restatement == the twin's state_dict, entry by entry, and the
    file's symbol bits are _huffman_total_bits of the records' histogram (CPU model, no kernel)."""
    import torch
    from oracle import configs
    from boosting_nerv_amd import codec, qstream
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.lib.entropy_model import huff_decode
    args = configs.tiny_nerv()
    args.__dict__.update(quant_model_bit=8, quant_embed_bit=6, crop_list="180_320", final_size=180 * 320, full_data_length=4)
    torch.manual_seed(3)
    model = T.build_model(args)
    (_, twin), records = T.quant_model(model, args)
    path = str(tmp_path / "tiny.bnrq")
    budget = codec.encode_posthoc(model, args, records, None, path)
    flat = torch.cat([r["quant"].flatten() for r in records.values()]).to(torch.int64)
    hist = torch.bincount(flat, minlength=1)
    assert budget["symbol_bits"] == T._huffman_total_bits(hist[hist > 0].tolist()) and budget["n_symbols"] == flat.numel()
    assert budget == qstream.info(path) and budget["total"] == 8 * os.path.getsize(path)
    qs = qstream.read(path)
    assert qs.settings["model"] == "NeRV_Boost" and qs.settings["huff_run"] == 256 and qs.settings["quant_model_bit"] == 8
    sym = huff_decode(qs.words, np.concatenate([r.run_bits for r in qs.records]), [r.count for r in qs.records], qs.lengths)
    sd = twin.state_dict()
    keys = [k for k in sd if "encoder" not in k]
    assert len(keys) == len(qs.records)
    at = 0
    for k, r in zip(keys, qs.records):
        got = Q.restate(sym[at:at + r.count], r.min, r.scale, r.outer, r.red, r.inner)
        assert got.tobytes() == sd[k].reshape(-1).numpy().tobytes(), k
        at += r.count
    assert "Huffman codes" in codec.describe_posthoc(budget) and codec.main(["info", path]) == budget
    with open(tmp_path / "other.bnrq", "wb") as f:          # a plain file object: the budget comes back all the same
        assert codec.encode_posthoc(model, args, records, None, f) == budget
    assert (tmp_path / "other.bnrq").read_bytes() == open(path, "rb").read()
