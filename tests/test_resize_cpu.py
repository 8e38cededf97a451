"""--resize_list on the host: the definition (boosting_nerv_amd/resize.py) against torch's antialiased bicubic, the
tables by hand, the loader, the parsers' refusals and the header key.  No GPU.

No number here comes from the code under test: the bound is the fp32 rounding of weights and sums that torch does and the float64 form
does not, (T_h + T_w + 4) * 2^-23 * L1 with L1 the product of the largest absolute row sums of the two tables (inputs in [0, 1]); the
hand-written rows are the Keys cubic (a = -0.5) evaluated in exact fractions."""
import io
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from boosting_nerv_amd import resize as R

from resize_cases import GEOMETRIES, IDS as _IDS, png_dir as _png_dir


def _input(H, W):
    return torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))


def _bound(H, W, h, w):
    th, tw = R.axis_table(H, h)[2], R.axis_table(W, w)[2]
    l1 = float(np.abs(th.astype(np.float64)).sum(axis=1).max() * np.abs(tw.astype(np.float64)).sum(axis=1).max())
    return (th.shape[1] + tw.shape[1] + 4) * 2.0 ** -23 * l1


@pytest.mark.parametrize("geom", GEOMETRIES, ids=_IDS)
def test_float64_definition_is_torchs_antialiased_bicubic(geom):
    H, W, h, w = geom
    x = _input(H, W)
    want = F.interpolate(x, (h, w), mode="bicubic", align_corners=False, antialias=True).double().numpy()
    got = R.resize_reference64(x.numpy(), (h, w), clamp=False)
    assert got.dtype == np.float64 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{geom}: |ref64 - torch| = {err:.3g}, bound {_bound(*geom):.3g}")
    assert err <= _bound(*geom)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=_IDS)
def test_fp32_definition_is_within_the_bound_of_the_float64_one(geom):
    H, W, h, w = geom
    x = _input(H, W)
    for clamp in (False, True):
        got = R.resize_reference(x.numpy(), (h, w), clamp=clamp)
        want = R.resize_reference64(x.numpy(), (h, w), clamp=clamp)
        assert got.dtype == np.float32 and got.shape == (2, 3, h, w)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{geom} clamp={clamp}: |ref32 - ref64| = {err:.3g}, bound {_bound(*geom):.3g}")
        assert err <= _bound(*geom)
    t = R.resize_reference(x, (h, w))                                # a tensor in, a tensor out, the same bits
    assert torch.is_tensor(t) and t.dtype == torch.float32 and np.array_equal(t.numpy(), R.resize_reference(x.numpy(), (h, w)))


def test_equal_size_returns_the_input_and_up_sampling_is_clamped():
    x = _input(9, 16)
    assert np.array_equal(R.resize_reference(x.numpy(), (9, 16)), x.numpy())
    assert np.array_equal(R.resize_reference(x.numpy(), (9, 16), clamp=False), x.numpy())
    x = _input(12, 20)
    raw, clamped = R.resize_reference(x.numpy(), (24, 40), clamp=False), R.resize_reference(x.numpy(), (24, 40))
    assert raw.min() < 0.0 and raw.max() > 1.0                          # the cubic's negative lobes overshoot ...
    assert clamped.min() >= 0.0 and clamped.max() <= 1.0 and np.array_equal(clamped, np.clip(raw, 0, 1))      # ... and the clamp is the last step


def _keys(x):
    """The Keys cubic, a = -1/2, in exact arithmetic."""
    x, a = abs(Fraction(x)), Fraction(-1, 2)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return Fraction(0)


def test_tables_by_hand():
    # 4 -> 2: scale 2, s = 2, centres 1 and 3.  Output 0: first = max(0, int(1 - 4 + .5)) = 0, end = min(int(1 + 4 + .5), 4) = 4,
    # arguments (j - 1 + .5) / 2 = -1/4, 1/4, 3/4, 5/4.  Output 1 mirrors it.
    w = [_keys(Fraction(v, 4)) for v in (-1, 1, 3, 5)]
    assert w == [Fraction(111, 128), Fraction(111, 128), Fraction(29, 128), Fraction(-9, 128)]
    row = np.array([float(v / sum(w)) for v in w])
    first, count, weights = R.axis_table(4, 2)
    assert first.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.float32
    assert first.tolist() == [0, 0] and count.tolist() == [4, 4] and weights.shape == (2, 4)
    assert np.array_equal(weights, np.stack([row, row[::-1]]).astype(np.float32))
    # 2 -> 4: scale 1/2, s = 1, centres 1/4, 3/4, 5/4, 7/4.  Every output reads both inputs: first = max(0, int(c - 1.5)) = 0,
    # end = min(int(c + 2.5), 2) = 2; arguments j - c + 1/2
    rows = []
    for c in (Fraction(1, 4), Fraction(3, 4), Fraction(5, 4), Fraction(7, 4)):
        w = [_keys(j - c + Fraction(1, 2)) for j in (0, 1)]
        rows.append([float(v / sum(w)) for v in w])
    first, count, weights = R.axis_table(2, 4)
    assert first.tolist() == [0] * 4 and count.tolist() == [2] * 4
    assert np.array_equal(weights, np.array(rows).astype(np.float32))
    assert rows[0] == [float(Fraction(37, 34)), float(Fraction(-3, 34))]
    # rows are zero-padded to the longest: 7 -> 3 has a border row shorter than the inner ones
    first, count, weights = R.axis_table(7, 3)
    assert count.min() < count.max() == weights.shape[1]
    for i in range(3):
        assert not weights[i, count[i]:].any() and abs(float(weights[i].astype(np.float64).sum()) - 1.0) < 4 * 2.0 ** -24 * weights.shape[1]
    assert R.axis_table(7, 3)[2] is weights                            # cached by (n_in, n_out)


def test_tap_limit_and_parse_refusals():
    assert R.axis_table(64, 1)[2].shape == (1, 64)
    with pytest.raises(ValueError, match="130 taps"):
        R.axis_table(130, 1)
    with pytest.raises(ValueError, match="taps"):
        R.resize_reference(np.zeros((1, 130, 4), dtype=np.float32), (1, 4))
    assert R.parse_resize("-1") is None and R.parse_resize("540_960") == (540, 960) and R.parse_resize(" 3_2 ") == (3, 2)
    for bad in ("", "540", "540x960", "540_960_3", "0_4", "-2", "a_b", "5_-3", "1.5_2"):
        with pytest.raises(ValueError, match="resize_list"):
            R.parse_resize(bad)


def test_device_table_layout():
    first, count, w = R.axis_table(36, 17)
    packed = R.pack_table(first, count, w)
    n, T = w.shape
    assert packed.dtype == np.int32 and packed.size == (2 + 2 * T) * n
    assert np.array_equal(packed[:n], first) and np.array_equal(packed[n:2 * n], count)
    assert np.array_equal(packed[2 * n:2 * n + n * T].view(np.float32).reshape(n, T), w)
    assert np.array_equal(packed[2 * n + n * T:].view(np.float32).reshape(T, n), w.T)
    # the LDS pitch of the row pass covers every strip's inputs from the 16-byte boundary below its first one
    for n_in, n_out in ((480, 320), (1920, 960), (64, 1), (20, 40), (1000, 67)):
        first, count, _ = R.axis_table(n_in, n_out)
        span = R.strip_span(first, count)
        assert span % 4 == 0
        for o in range(0, n_out, R.STRIP):
            assert int((first[o:o + R.STRIP] + count[o:o + R.STRIP]).max()) - (int(first[o]) & ~3) <= span


# ---------------------------------------------------------------------------------------------------------------------- the loader
def test_frame_hw_follows_the_flag():
    from boosting_nerv_amd.hnerv_utils import frame_hw
    assert frame_hw(SimpleNamespace(crop_list="270_480")) == (270, 480)
    assert frame_hw(SimpleNamespace(crop_list="270_480", resize_list="-1")) == (270, 480)
    assert frame_hw(SimpleNamespace(crop_list="270_480", resize_list="180_320")) == (180, 320)
    with pytest.raises(ValueError, match="resize_list"):
        frame_hw(SimpleNamespace(crop_list="270_480", resize_list="180"))


@pytest.mark.parametrize("source", ["png", "synthetic"])
def test_dataset_resizes_after_the_crop(tmp_path, source):
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    data_path = _png_dir(tmp_path / "frames", 3, 40, 60) if source == "png" else "synthetic:3x36x48"
    plain = VideoDataSet(SimpleNamespace(data_path=data_path, crop_list="36_48"))
    off = VideoDataSet(SimpleNamespace(data_path=data_path, crop_list="36_48", resize_list="-1"))
    on = VideoDataSet(SimpleNamespace(data_path=data_path, crop_list="36_48", resize_list="24_32"))
    assert plain.resize is None and off.resize is None and on.resize == (24, 32)
    assert plain.final_size == off.final_size == 36 * 48 and on.final_size == 24 * 32 and len(on) == 3
    for i in range(3):
        full = plain[i]["img"]
        assert full.shape == (3, 36, 48) and torch.equal(off[i]["img"], full)          # -1: the frames of a run without the flag, bit for bit
        got = on[i]
        assert got["img"].shape == (3, 24, 32) and got["img"].dtype == torch.float32 and got["norm_idx"] == plain[i]["norm_idx"]
        assert torch.equal(got["img"], R.resize_reference(full, (24, 32)))               # crop, then resize
    if source == "png":                 # the crop is the centre crop of the 40x60 file, as before
        from PIL import Image
        a = np.asarray(Image.open(os.path.join(data_path, "f000.png")))[2:38, 6:54]
        assert torch.equal(plain[0]["img"], torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255))
    with pytest.raises(ValueError, match="taps"):                       # over the tap limit: refused when the dataset is built
        VideoDataSet(SimpleNamespace(data_path="synthetic:2x170x48", crop_list="170_48", resize_list="1_48"))


def test_yuv_dataset_resizes_on_the_host(tmp_path):
    from boosting_nerv_amd import yuvio
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    rng = np.random.default_rng(5)
    path = str(tmp_path / "clip_16x12_8bit.yuv")
    yuvio.write(path, [(rng.integers(16, 236, size=(12, 16), dtype=np.uint8), rng.integers(16, 241, size=(6, 8), dtype=np.uint8),
                        rng.integers(16, 241, size=(6, 8), dtype=np.uint8)) for _ in range(2)])
    plain = VideoDataSet(SimpleNamespace(data_path=path, crop_list="10_12"))
    on = VideoDataSet(SimpleNamespace(data_path=path, crop_list="10_12", resize_list="5_8"))
    assert on.final_size == 40
    for i in range(2):
        assert torch.equal(on[i]["img"], R.resize_reference(plain[i]["img"], (5, 8)))


# ---------------------------------------------------------------------------------------------------------------------- the parsers
_YUV = "--data_path clip_480x270_8bit.yuv --crop_list 270_480"


@pytest.mark.parametrize("script", ["train_nerv_all", "train_nerv_compression"])
def test_parsers_refuse_what_a_resized_run_cannot_honour(script):
    import importlib
    mod = importlib.import_module(f"boosting_nerv_amd.{script}")
    a = mod.parse_args((_YUV + " --resize_list 180_320").split())
    assert a.resize_list == "180_320"
    assert mod.parse_args((_YUV + " --yuv_loss 1").split()).yuv_loss == 1.0             # (without the flag the plane loss parses)
    for flags in ("--yuv_loss 1", "--yuv_msssim 50", "--loss YUV420"):
        with pytest.raises(ValueError, match="resize_list"):
            mod.parse_args((_YUV + f" --resize_list 180_320 {flags}").split())
    with pytest.raises(ValueError, match="embed_inter"):
        mod.parse_args((_YUV + " --resize_list 180_320 --interpolation --embed_inter").split())
    with pytest.raises(ValueError, match="resize_list"):
        mod.parse_args((_YUV + " --resize_list 180x320").split())
    assert mod.parse_args((_YUV + " --resize_list -1 --interpolation --embed_inter").split()).embed_inter


# ---------------------------------------------------------------------------------------------------------------------- the header key
def _posthoc_file(tmp_path, name, **over):
    from oracle import configs
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    args = configs.tiny_nerv()
    args.__dict__.update(quant_model_bit=8, quant_embed_bit=6, crop_list="270_480", final_size=180 * 320, full_data_length=4)
    args.__dict__.update(over)
    torch.manual_seed(3)
    model = T.build_model(args)
    _, records = T.quant_model(model, args)
    path = str(tmp_path / name)
    return path, codec.encode_posthoc(model, args, records, None, path)


def test_posthoc_header_carries_source_crop_only_under_the_flag(tmp_path):
    from boosting_nerv_amd import codec, qstream
    on, budget_on = _posthoc_file(tmp_path, "on.bnrq", resize_list="180_320")
    s = qstream.read(on).settings
    assert s["crop_list"] == "180_320" and s["source_crop"] == "270_480" and s["final_size"] == 180 * 320
    assert budget_on["total"] == 8 * os.path.getsize(on)
    info = codec.main(["info", on])
    assert info["source_crop"] == "270_480" and {k: v for k, v in info.items() if k != "source_crop"} == budget_on
    assert "source_crop 270_480" in codec.describe_any(info)
    # without the flag (absent, or -1): no key, and the bytes a run wrote before -- those of the same settings at the crop size
    absent, budget = _posthoc_file(tmp_path, "absent.bnrq", crop_list="180_320")
    minus1, _ = _posthoc_file(tmp_path, "minus1.bnrq", crop_list="180_320", resize_list="-1")
    assert open(absent, "rb").read() == open(minus1, "rb").read()
    s = qstream.read(absent).settings
    assert "source_crop" not in s and s["crop_list"] == "180_320"
    assert codec.main(["info", absent]) == budget and "source_crop" not in budget
    # the key is all the flag adds: the header grows by its JSON text, nothing else moves
    assert budget_on["total"] - budget["total"] == budget_on["header"] - budget["header"] > 0
    assert all(budget_on[k] == budget[k] for k in budget if k not in ("total", "header", "bytes", "padding"))


def test_cem_header_carries_source_crop_only_under_the_flag():
    from oracle import configs
    from boosting_nerv_amd import bitstream, codec
    rng = np.random.default_rng(7)
    sym = np.rint(rng.normal(1.5, 9.0, size=4095)).astype(np.int32).clip(-128, 127)
    rec = codec._code_symbols(torch.from_numpy(sym), sym.mean(), sym.std(ddof=1), 0.0123)
    raw = [rng.normal(size=17).astype(np.float32)]
    blobs = {}
    for name, over in (("absent", {}), ("minus1", {"resize_list": "-1"}), ("on", {"resize_list": "180_320"})):
        args = configs.tiny_nerv()
        args.__dict__.update(crop_list="270_480", **over)
        settings = codec._settings(args, 3, codec._frame_hw(args, None, None))
        blobs[name] = bitstream.to_bytes(settings, [rec], (), None, raw)
    assert blobs["absent"] == blobs["minus1"]
    s = bitstream.read(blobs["absent"]).settings
    assert "source_crop" not in s and s["crop_list"] == "270_480" and s["final_size"] == 270 * 480
    s = bitstream.read(blobs["on"]).settings
    assert s["source_crop"] == "270_480" and s["crop_list"] == "180_320" and s["final_size"] == 180 * 320
    info = codec.info(io.BytesIO(blobs["on"]))
    assert info["source_crop"] == "270_480" and info["total"] == 8 * len(blobs["on"]) == 8 * info["bytes"]
    plain = codec.info(blobs["absent"])
    assert "source_crop" not in plain and plain == bitstream.info(blobs["absent"]) and plain["total"] == 8 * len(blobs["absent"])
