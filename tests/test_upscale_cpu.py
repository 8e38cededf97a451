"""The up-scaling decode on the host: that the seeded inputs of test_gpu_upscale.py qualify for the code rule, the ABI of
bnerv_resize_cols_yuv420 and what it rejects without a device, the --upscale flag, and the refusals of Decoder / score.  No GPU.

The share bound is a condition on the inputs, computed from the float64 restatement alone (tests/test_gpu_yuv.py: TIE_SHARE)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from boosting_nerv_amd import yuvio

import upscale_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", U.op_cases(), ids=U.case_id)
def test_inputs_of_the_gpu_test_stay_clear_of_rounding_ties(case):
    k, B, depth, matrix, rng = case
    (h, w), (H, W) = U.GEOMETRIES[k]
    x = U.case_input(k, B, depth)
    assert tuple(x.shape) == (B, 3, h, w) and x.dtype == torch.float32
    rgb = U.case_resized(k, B, depth)
    assert rgb.shape == (B, 3, H, W) and rgb.dtype == np.float32 and rgb.min() >= 0.0 and rgb.max() <= 1.0
    want, near = U.tie_split(rgb, yuvio.coefficients(matrix, rng, depth))
    share = float(near.mean())
    print(f"  {U.case_id(case)}: {want.size} samples, {share:.4%} in the tie window")
    if want.size >= U.SHARE_MIN_SAMPLES:
        assert share < U.TIE_SHARE, share
        assert float(x.min()) < 0.0 and float(x.max()) > 1.0 and rgb.min() == 0.0 and rgb.max() == 1.0      # both clamps are hit


def test_which_cases_carry_the_share_condition():
    """k = 0 .. 2 never reach SHARE_MIN_SAMPLES; every other geometry does at B = 3, and all but 18 x 30 (810 samples) at B = 1."""
    sizes = {(k, B): B * 3 * H * W // 2 for k, (_, (H, W)) in enumerate(U.GEOMETRIES) for B in U.BATCHES}
    small = sorted(key for key, n in sizes.items() if n < U.SHARE_MIN_SAMPLES)
    assert small == [(0, 1), (0, 3), (1, 1), (1, 3), (2, 1), (2, 3), (5, 1)], small
    assert U.GEOMETRIES[U.IDENTITY][0] == U.GEOMETRIES[U.IDENTITY][1]


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_symbol_is_declared_listed_and_bound():
    from boosting_nerv_amd import _lib as L, ops
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    assert re.search(r"^int bnerv_resize_cols_yuv420\(void\* stream, const float\* x, const void\* table_dev, int B, int n_in, int H, int W, int T, "
                     r"void\* out,\s+int bytes_per_sample, size_t frame_stride_bytes, const bnerv_yuv_coeffs\* coeffs\);", header, re.M)
    assert "#define BNERV_ABI_VERSION 9" in header and L.ABI_VERSION == 9
    res, args = L.SYMBOLS["bnerv_resize_cols_yuv420"]
    assert res is C.c_int and len(args) == 12
    lib = L.load()
    assert lib.bnerv_abi_version() == 9 and lib.bnerv_resize_cols_yuv420.argtypes == args
    assert callable(ops.resize_to_yuv420)
    assert "upyuv" in open(os.path.join(ROOT, "boosting_nerv_amd", "csrc", "build.sh")).read()


def test_entry_point_validates_before_any_launch():
    """Every rejected argument returns BNERV_E_ARG (-1) with a message, with no GPU in the machine."""
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    k = yuvio.coefficients("bt709", "limited", 8).store_struct()
    kp, one = C.byref(k), C.c_void_p(64)

    def call(x=one, tab=one, B=1, n_in=2, H=4, W=4, T=4, out=one, bps=1, stride=24, coeffs=kp):
        return lib.bnerv_resize_cols_yuv420(None, x, tab, B, n_in, H, W, T, out, bps, stride, coeffs)

    for bad in (dict(x=None), dict(tab=None), dict(out=None), dict(coeffs=None)):
        assert call(**bad) == -1 and b"resize_cols_yuv420: null" in lib.bnerv_last_error(), bad
    for bad in (dict(x=C.c_void_p(66)), dict(tab=C.c_void_p(66))):
        assert call(**bad) == -1 and b"4-byte aligned" in lib.bnerv_last_error(), bad
    for bad in (dict(H=3), dict(W=3), dict(H=5, W=5, stride=64)):
        assert call(**bad) == -1 and b"even" in lib.bnerv_last_error(), bad
    for T in (0, -1, 65):
        assert call(T=T) == -1 and b"taps" in lib.bnerv_last_error(), T
    for bad in (dict(stride=23), dict(bps=2, stride=46), dict(stride=0)):
        assert call(**bad) == -1 and b"smaller than a frame" in lib.bnerv_last_error(), bad
    for bad in (dict(bps=2, stride=49), dict(bps=2, stride=48, out=C.c_void_p(65))):
        assert call(**bad) == -1 and b"odd address" in lib.bnerv_last_error(), bad
    for bps in (0, 3):
        assert call(bps=bps) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    for bad in (dict(B=0), dict(B=65536), dict(n_in=0), dict(H=0), dict(W=-2)):
        assert call(**bad) == -1, bad


# ---------------------------------------------------------------------------------------------------------------------- the flag
@pytest.mark.parametrize("cmd", [["decode", "f.bnrq", "--out", "o"], ["psnr", "f.bnrq", "--ref", "r.yuv"], ["score", "f.bnrq", "--ref", "r.yuv"]],
                         ids=["decode", "psnr", "score"])
def test_parser_takes_upscale_with_and_without_a_value(cmd):
    from boosting_nerv_amd import codec
    p = codec.build_parser()
    assert p.parse_args(cmd).upscale is None
    assert p.parse_args(cmd + ["--upscale"]).upscale is True
    assert p.parse_args(cmd + ["--upscale", "--no_graph"]).upscale is True
    assert p.parse_args(cmd + ["--upscale", "1920x1080"]).upscale == (1080, 1920)      # WxH on the command line, (H, W) inside
    for bad in ("1080", "1920_1080", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(cmd + ["--upscale", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["info", "f.bnrq", "--upscale"])


# ---------------------------------------------------------------------------------------------------------------------- refusals
def _posthoc_file(tmp_path, name, **over):
    """The recipe of tests/test_resize_cpu.py: a tiny NeRV model as a post-hoc file, written on the host."""
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
    codec.encode_posthoc(model, args, records, None, path)
    return path


def test_resolve_upscale():
    from boosting_nerv_amd import codec
    resized = {"source_crop": "270_480"}
    assert codec.resolve_upscale(None, resized, (180, 320)) is None
    assert codec.resolve_upscale(True, resized, (180, 320), "yuv420p") == (270, 480)
    assert codec.resolve_upscale((360, 640), {}, (180, 320), "yuv420p10le") == (360, 640)
    assert codec.resolve_upscale([271, 481], {}, (180, 320)) == (271, 481)             # rgb8 packs any size
    with pytest.raises(ValueError, match="source_crop"):
        codec.resolve_upscale(True, {}, (180, 320))
    for size in ((271, 480), (270, 481)):
        with pytest.raises(ValueError, match="even"):
            codec.resolve_upscale(size, {}, (180, 320), "yuv420p")
    with pytest.raises(ValueError, match="even"):
        codec.resolve_upscale(True, {"source_crop": "271_480"}, (180, 320), "yuv420p")
    for bad in ((270,), (270, 480, 3), (0, 480), "big", (270.5, 480), 480):
        with pytest.raises(ValueError, match="upscale"):
            codec.resolve_upscale(bad, resized, (180, 320))
    with pytest.raises(ValueError, match="taps"):                                       # the vertical pass would need 180 taps
        codec.resolve_upscale((2, 320), {}, (180, 320), "yuv420p")


def test_decoder_refuses_before_it_touches_a_device(tmp_path, monkeypatch):
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T

    def no_model(*a, **k):
        raise AssertionError("the refusal comes before the model is built")
    plain = _posthoc_file(tmp_path, "plain.bnrq", crop_list="180_320")
    resized = _posthoc_file(tmp_path, "resized.bnrq", resize_list="180_320")
    monkeypatch.setattr(T, "build_model", no_model)
    with pytest.raises(ValueError, match="source_crop"):
        codec.Decoder(plain, "cuda", upscale=True)
    with pytest.raises(ValueError, match="even"):
        codec.Decoder(plain, "cuda", pack="yuv420p", upscale=(271, 480))
    with pytest.raises(ValueError, match="upscale"):
        codec.Decoder(resized, "cuda", upscale=(270, 480, 1))
    with pytest.raises(AssertionError, match="before the model"):                        # (the sizes that pass go on to the model)
        codec.Decoder(resized, "cuda", pack="yuv420p", upscale=True)


def test_score_refuses_an_odd_window_offset(tmp_path):
    """A 274 x 482 source: the centre crop of 270 x 480 starts at row 2, column 1.  `codec psnr` rounds such an offset down for a file at the
    crop's own size; for an up-scaled frame that would score another picture, so it is refused, before any launch."""
    from boosting_nerv_amd import codec
    assert codec.score_window((270, 480), (270, 480)) == (0, 0) and codec.score_window((274, 484), (270, 480)) == (2, 2)
    for src in ((274, 482), (272, 484), (272, 482)):
        with pytest.raises(ValueError, match="even row and column"):
            codec.score_window(src, (270, 480))
    with pytest.raises(NotImplementedError):                                             # (the loader's refusal of a source smaller than the crop stands)
        codec.score_window((180, 320), (270, 480))
    path = str(tmp_path / "src_482x274_8bit.yuv")
    grey = (np.full((274, 482), 128, np.uint8), np.full((137, 241), 128, np.uint8), np.full((137, 241), 128, np.uint8))
    yuvio.write(path, [grey, grey])
    ref = yuvio.YuvFile(path)

    def launched(*a, **k):
        raise AssertionError("score launched before it refused")
    dec = SimpleNamespace(upscale=(270, 480), out_hw=(270, 480), frame_hw=(180, 320), n_frames=2, pack="yuv420p", settings={"source_crop": "270_480"},
                          coeffs=yuvio.coefficients("bt709", "limited", 8), device=torch.device("cpu"), _launch=launched)
    dec._need_pack = codec.Decoder._need_pack.__get__(dec)
    with pytest.raises(ValueError, match="even row and column"):
        codec.Decoder.score(dec, ref)
