"""The compression bitstream on the host: container round trip through the range-ANS coder of the library, the bit budget, the
rejection of damaged files, and the C symbols of the decoder's kernels."""
import io
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("bnerv_dequant_table", "bnerv_frame_to_u8")


def _record(sym, mean, std, scale, beta=None):
    """What codec.encode does with a tensor's symbols: the encoder's range rule (hi = lo + 1 for a constant tensor), the clamped std."""
    from boosting_nerv_amd.bitstream import Record
    from boosting_nerv_amd.lib.entropy_model import ans_encode_gaussian
    sym = np.asarray(sym, dtype=np.int32)
    lo, hi = int(sym.min()), int(sym.max())
    if lo == hi:
        hi = lo + 1
    mean, std = np.float32(mean), np.float32(np.clip(np.float32(std), 1e-5, 1e10))
    words = ans_encode_gaussian(sym, lo, hi, float(mean), float(std))
    return Record(sym.size, np.float32(scale), mean, std, lo, hi, words, None if beta is None else np.float32(beta))


def _synthetic():
    rng = np.random.default_rng(7)
    syms = []
    for n in (1, 2, 4095, 70001):
        s = np.rint(rng.normal(1.5, 9.0, size=n)).astype(np.int32).clip(-128, 127)
        syms.append(s)
    syms[2][5], syms[2][77] = -128, 127                     # the ends of the 8-bit range
    syms[3][0], syms[3][-1] = 127, -128
    syms.append(np.full(300, -3, dtype=np.int32))           # a constant tensor: lo == hi -> hi = lo + 1
    tensors = [_record(s, s.mean(), s.std(ddof=1) if s.size > 1 else 0.0, 0.0123 * (i + 1)) for i, s in enumerate(syms)]
    esyms = [rng.integers(0, 256, size=4 * 9 * 16).astype(np.int32) for _ in range(3)]
    embeds = [_record(s, s.mean(), s.std(ddof=1), 0.031, beta=-1.25) for s in esyms]
    raw = [rng.normal(size=17).astype(np.float32), np.array([np.float32(1e-30), np.float32(-0.0)], dtype=np.float32)]
    settings = {"model": "HNeRV_Boost", "fc_dim": 10, "enc_dim": "16_4", "final_size": 180 * 320, "full_data_length": 3, "crop_list": "180_320",
                "dec_strds": [5, 2, 2]}
    return settings, syms, tensors, esyms, embeds, raw


def _file(**over):
    from boosting_nerv_amd import bitstream as B
    settings, syms, tensors, esyms, embeds, raw = _synthetic()
    buf = io.BytesIO()
    n = B.write(buf, settings, tensors, embeds, (4, 9, 16), raw)
    assert n == len(buf.getvalue())
    return buf.getvalue(), (settings, syms, tensors, esyms, embeds, raw)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_round_trip_symbols_fields_and_budget():
    from boosting_nerv_amd import bitstream as B
    from boosting_nerv_amd.lib.entropy_model import ans_decode_gaussian
    blob, (settings, syms, tensors, esyms, embeds, raw) = _file()
    bs = B.read(io.BytesIO(blob))
    assert bs.settings == settings and bs.embed_shape == (4, 9, 16)
    assert len(bs.tensors) == len(tensors) == 5 and len(bs.embeds) == 3 and len(bs.raw) == 2
    assert tensors[4].lo == -3 and tensors[4].hi == -2 and tensors[2].lo == -128 and tensors[2].hi == 127
    for got, want, sym in zip(list(bs.tensors) + list(bs.embeds), tensors + embeds, syms + esyms):
        assert (got.count, got.lo, got.hi) == (want.count, want.lo, want.hi)
        for f in ("scale", "mean", "std"):
            assert getattr(got, f).dtype == np.float32 and _bits(getattr(got, f)) == _bits(getattr(want, f)), f
        assert (got.beta is None) == (want.beta is None) and (want.beta is None or _bits(got.beta) == _bits(want.beta))
        assert got.words.dtype == np.uint32 and np.array_equal(got.words, want.words)
        dec = ans_decode_gaussian(got.words, got.count, got.lo, got.hi, float(got.mean), float(got.std))
        assert np.array_equal(dec, sym)
    for got, want in zip(bs.raw, raw):
        assert np.array_equal(_bits(got), _bits(want))                     # bit-equal, the sign of zero included
    budget = B.info(blob)
    items = ("tensor_words", "tensor_side", "embed_words", "embed_side", "raw", "header")
    assert budget["total"] == 8 * len(blob) == sum(budget[k] for k in items) and budget["bytes"] == len(blob)
    assert budget["tensor_words"] == 32 * sum(r.words.size for r in tensors) and budget["embed_words"] == 32 * sum(r.words.size for r in embeds)
    assert budget["coded_words"] == budget["tensor_words"] + budget["embed_words"]
    assert budget["tensor_side"] == 5 * 7 * 32 and budget["embed_side"] == 3 * 8 * 32 and budget["raw"] == (2 + 17 + 2) * 32
    assert (budget["n_tensors"], budget["n_embeds"], budget["n_raw"]) == (5, 3, 2)


def test_file_and_buffer_forms_agree(tmp_path):
    from boosting_nerv_amd import bitstream as B
    blob, (settings, _, tensors, _, embeds, raw) = _file()
    path = tmp_path / "clip.bnrv"
    assert B.write(str(path), settings, tensors, embeds, (4, 9, 16), raw) == len(blob)
    assert path.read_bytes() == blob
    assert B.info(str(path)) == B.info(blob) == B.info(io.BytesIO(blob))
    with open(path, "rb") as f:
        assert B.read(f).settings == settings
    # a stream without embeddings (NeRV_Boost, ENeRV_Boost)
    blob2 = B.to_bytes(settings, tensors, raw=raw)
    bs2 = B.read(blob2)
    assert bs2.embeds == [] and bs2.embed_shape is None and B.info(blob2)["embed_words"] == 0 and B.info(blob2)["total"] == 8 * len(blob2)


def test_rejects_bad_magic_and_bumped_version():
    from boosting_nerv_amd import bitstream as B
    blob, _ = _file()
    with pytest.raises(ValueError, match="magic"):
        B.read(b"XNRV" + blob[4:])
    bumped = blob[:4] + struct.pack("<I", B.VERSION + 1) + blob[8:]
    with pytest.raises(ValueError, match="version"):
        B.read(bumped)
    with pytest.raises(ValueError, match="version"):
        B.info(bumped)


@pytest.mark.parametrize("where", ["prefix", "middle", "last_byte"])
def test_rejects_truncated_file(where):
    from boosting_nerv_amd import bitstream as B
    blob, _ = _file()
    cut = {"prefix": 9, "middle": len(blob) // 2, "last_byte": len(blob) - 1}[where]
    with pytest.raises(ValueError, match="truncated"):
        B.read(blob[:cut])
    with pytest.raises(ValueError, match="truncated"):
        B.read(io.BytesIO(blob[:cut]))


def test_rejects_flipped_payload_byte():
    from boosting_nerv_amd import bitstream as B
    blob, _ = _file()
    for pos in (16, len(blob) // 2, len(blob) - 5):         # first payload byte, inside the coded words, last payload byte
        bad = bytearray(blob)
        bad[pos] ^= 0x10
        with pytest.raises(ValueError, match="CRC"):
            B.read(bytes(bad))


def test_new_symbols_are_declared_bound_and_exported():
    from boosting_nerv_amd import _lib
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    assert int(re.search(r"#define\s+BNERV_DEQUANT_CHUNK\s+(\d+)", header).group(1)) == _lib.DEQUANT_CHUNK
    lib = _lib.load()                                    # (binds every name of SYMBOLS: a missing export raises here)
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.bnerv_abi_version() == 9
    from boosting_nerv_amd import ops
    assert callable(ops.dequant_table) and callable(ops.frame_to_u8)


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(64)        # a non-null aligned address that is never dereferenced: every call below fails its checks first
    assert lib.bnerv_dequant_table(None, None) == -1 and b"dequant_table" in lib.bnerv_last_error()
    ck = L.DequantChunk()
    assert lib.bnerv_dequant_table(None, C.byref(ck)) == -1                      # no items
    ck.n_items = L.CEM_MAX_TENSORS + 1
    assert lib.bnerv_dequant_table(None, C.byref(ck)) == -1
    ck.n_items = 1
    ck.it[0].q, ck.it[0].out, ck.it[0].scale, ck.it[0].n = 64, 64, None, 4
    assert lib.bnerv_dequant_table(None, C.byref(ck)) == -1 and b"incomplete" in lib.bnerv_last_error()
    ck.it[0].scale, ck.it[0].n = 64, 0
    assert lib.bnerv_dequant_table(None, C.byref(ck)) == -1
    ck.it[0].n, ck.it[0].out = 4, 66
    assert lib.bnerv_dequant_table(None, C.byref(ck)) == -1 and b"4-byte" in lib.bnerv_last_error()
    assert lib.bnerv_frame_to_u8(None, None, one, 1, 2, 2) == -1 and b"frame_to_u8" in lib.bnerv_last_error()
    assert lib.bnerv_frame_to_u8(None, one, None, 1, 2, 2) == -1
    assert lib.bnerv_frame_to_u8(None, one, one, 0, 2, 2) == -1 and lib.bnerv_frame_to_u8(None, one, one, 1, 0, 2) == -1
    assert lib.bnerv_frame_to_u8(None, one, one, 70000, 2, 2) == -1
    assert lib.bnerv_frame_to_u8(None, C.c_void_p(66), one, 1, 2, 2) == -1 and b"4-byte" in lib.bnerv_last_error()


def test_encode_refuses_the_hnerv_baseline_before_any_device_work():
    """codec.encode on --model HNeRV: the baseline has no quantised form on this path."""
    import torch
    from types import SimpleNamespace
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    with pytest.raises(NotImplementedError, match="HNeRV"):
        codec.encode(torch.nn.Linear(2, 2), DiffEntropyModel("gaussian"), SimpleNamespace(model="HNeRV"), None, io.BytesIO())
