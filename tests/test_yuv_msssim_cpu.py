"""The MS-SSIM-Y term without a GPU: the new symbols, what the two entry points reject before any launch, the float64
restatement yuvio.luma_pre_reference against the store restatement and against autograd, the command-line flag and its refusals, and the
record the steps take."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from boosting_nerv_amd import yuvio

NEW_SYMBOLS = ("bnerv_yuv_luma_pair", "bnerv_luma_grad_rgb")


def _planes(gen, B, h, w, depth):
    top = 2 ** depth
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    return (gen.integers(0, top, (B, h, w)).astype(dt), gen.integers(0, top, (B, h // 2, w // 2)).astype(dt),
            gen.integers(0, top, (B, h // 2, w // 2)).astype(dt))


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    import os
    import re
    from boosting_nerv_amd import _lib as L, ops
    lib = L.load()
    assert lib.bnerv_abi_version() == 9 and L.ABI_VERSION == 9          # additive
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and re.search(rf"\bint {name}\(", header), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(L.SYMBOLS[name][1])
    for name in ("yuv_luma_pair", "luma_grad_rgb", "yuv420_msssim_value_grad_stats", "yuv420_msssim_loss"):
        assert callable(getattr(ops, name)), name
    assert ops.MSSSIM_MIN_SIDE == 160


def test_luma_pair_validates_before_any_launch():
    """Every rejected argument returns BNERV_E_ARG (-1) with a message, with no GPU in the machine."""
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    k = yuvio.coefficients("bt709", "limited", 8).store_struct()
    kp, one = C.byref(k), C.c_void_p(64)

    def pair(pred=one, B=1, H=2, W=2, src=one, bps=1, stride=6, n_frames=1, src_h=2, src_w=2, top=0, left=0, sel=None, coeffs=kp, yp=one, ys=one):
        return lib.bnerv_yuv_luma_pair(None, pred, B, H, W, src, bps, stride, n_frames, src_h, src_w, top, left, sel, coeffs, yp, ys)

    for bad in (dict(pred=None), dict(src=None), dict(coeffs=None), dict(yp=None), dict(ys=None)):
        assert pair(**bad) == -1 and b"yuv_luma_pair: null" in lib.bnerv_last_error(), bad
    for bps in (0, 3, 4):
        assert pair(bps=bps) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    big = dict(src_h=8, src_w=8, stride=96)
    for bad in (dict(top=7), dict(left=7), dict(H=10), dict(W=10), dict(top=-1), dict(left=-1), dict(top=2 ** 31 - 2)):
        assert pair(**big, **bad) == -1 and b"leaves" in lib.bnerv_last_error(), bad
    assert pair(stride=5) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert pair(bps=2, stride=11) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert pair(bps=2, stride=13) == -1 and b"odd" in lib.bnerv_last_error()
    assert pair(B=2) == -1 and b"without frame_sel" in lib.bnerv_last_error()      # two samples, one frame, no selector
    for bad in (dict(B=0), dict(B=70000, sel=one), dict(H=0), dict(W=0), dict(n_frames=0), dict(src_h=3), dict(src_w=3)):
        assert pair(**bad) == -1, bad
    for bad in (dict(pred=C.c_void_p(66)), dict(yp=C.c_void_p(66)), dict(ys=C.c_void_p(66)), dict(sel=C.c_void_p(66))):
        assert pair(**bad) == -1 and b"4-byte" in lib.bnerv_last_error(), bad


def test_luma_grad_rgb_validates_before_any_launch():
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    one, k3 = C.c_void_p(64), (C.c_double * 3)(0.2, 0.6, 0.06)

    def scatter(gy=one, B=1, H=2, W=2, k=k3, grad=one, term=one, loss=one):
        return lib.bnerv_luma_grad_rgb(None, gy, B, H, W, k, 1.0, grad, 0, term, loss)

    for bad in (dict(k=None), dict(term=None), dict(loss=None), dict(gy=None), dict(grad=None)):     # (gy and grad may only be null together)
        assert scatter(**bad) == -1 and b"luma_grad_rgb: null" in lib.bnerv_last_error(), bad
    for bad in (dict(B=0), dict(B=70000), dict(H=0), dict(W=0), dict(H=1 << 15, W=1 << 15)):
        assert scatter(**bad) == -1, bad
    for bad in (dict(gy=C.c_void_p(66)), dict(grad=C.c_void_p(66)), dict(term=C.c_void_p(66)), dict(loss=C.c_void_p(66))):
        assert scatter(**bad) == -1 and b"4-byte" in lib.bnerv_last_error(), bad


# ---------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (18, 34)])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix,rng_name", [("bt709", "limited"), ("bt601", "limited"), ("bt709", "full")])
def test_pre_is_the_store_restatements_luma_exactly(hw, depth, matrix, rng_name):
    """The value Yp is the quotient of IS to_yuv_reference's luma `pre`, bit for bit, for P in [0, 1]; Yp is that value divided by the peak
    (the division rounds once, so the product maxcode * Yp gives it back only to an ulp: 0.2 % of the elements differ in the last bit)."""
    gen = np.random.default_rng(hw[0] * 100 + depth)
    c = yuvio.coefficients(matrix, rng_name, depth)
    P = gen.random((2, 3) + hw)
    planes = _planes(gen, 2, hw[0] + 2, hw[1] + 4, depth)
    Yp, Ys, k, pre = yuvio.luma_pre_reference(P, planes, c, (1, 3), return_pre=True)
    _, ref = yuvio.to_yuv_reference(P, c, return_pre=True)
    assert pre.dtype == np.float64 and np.array_equal(pre[:, 0], ref[0])
    assert np.array_equal(Yp, pre / c.maxcode)
    assert np.all(np.abs(c.maxcode * Yp[:, 0] - ref[0]) <= np.spacing(ref[0]))
    assert Ys.dtype == np.float64 and np.array_equal(Ys[:, 0], planes[0][:, 1:1 + hw[0], 3:3 + hw[1]] / float(c.maxcode))
    three = yuvio.luma_pre_reference(P, planes, c, (1, 3))
    assert len(three) == 3 and np.array_equal(three[0], Yp) and np.array_equal(three[2], k)


@pytest.mark.parametrize("depth,matrix,rng_name", [(8, "bt709", "limited"), (10, "bt601", "full")])
def test_k_is_the_autograd_gradient_of_the_formula(depth, matrix, rng_name):
    import torch
    gen = np.random.default_rng(11)
    c = yuvio.coefficients(matrix, rng_name, depth)
    P = gen.uniform(-0.25, 1.25, (2, 3, 6, 10))
    planes = _planes(gen, 2, 6, 10, depth)
    Yp, _, k = yuvio.luma_pre_reference(P, planes, c)
    Pt = torch.tensor(P, requires_grad=True)
    M = torch.tensor(c.to_yuv)
    Yt = (float(c.offset[0]) + float(c.denom[0]) * (M[0, 0] * Pt[:, 0] + M[0, 1] * Pt[:, 1] + M[0, 2] * Pt[:, 2])) / float(c.maxcode)
    assert np.allclose(Yp[:, 0], Yt.detach().numpy(), rtol=1e-15, atol=0)
    w = torch.tensor(gen.standard_normal((2, 6, 10)))
    (Yt * w).sum().backward()
    g = Pt.grad.numpy()
    for ch in range(3):
        want = g[:, ch] / w.numpy()
        assert np.all(np.abs(want - k[ch]) <= 1e-12 * abs(k[ch])), ch
    from boosting_nerv_amd import ops
    assert ops.luma_grad_consts(c) == tuple(float(v) for v in k)


def test_reference_refuses_windows_that_leave_the_frame():
    c = yuvio.coefficients()
    P, planes = np.zeros((1, 3, 2, 2)), _planes(np.random.default_rng(0), 1, 4, 4, 8)
    yuvio.luma_pre_reference(P, planes, c, (1, 1))                       # any parity
    for window in ((3, 0), (0, 3), (-1, 0)):
        with pytest.raises(ValueError):
            yuvio.luma_pre_reference(P, planes, c, window)
    with pytest.raises(ValueError):
        yuvio.luma_pre_reference(np.zeros((1, 2, 2, 2)), planes, c)


# ---------------------------------------------------------------------------------------------------------------------- flags
BASE = "--data_path clip_320x180_8bit.yuv --crop_list 180_320"


@pytest.mark.parametrize("which", ["train_nerv_all", "train_nerv_compression"])
def test_train_parsers_take_the_flag_and_refuse_what_no_run_can_honour(which):
    import importlib
    mod = importlib.import_module(f"boosting_nerv_amd.{which}")
    a = mod.parse_args([])
    assert a.yuv_msssim == 0 and a.yuv_loss == 0                        # off by default
    a = mod.parse_args(f"{BASE} --yuv_msssim 50".split())
    assert a.yuv_msssim == 50.0 and a.yuv_loss == 0                     # without --yuv_loss
    a = mod.parse_args(f"{BASE} --yuv_msssim 50 --yuv_loss 2".split())
    assert a.yuv_msssim == 50.0 and a.yuv_loss == 2.0                   # with it
    a = mod.parse_args(f"{BASE} --loss YUV420 --yuv_msssim 50".split())
    assert a.loss == "YUV420" and a.yuv_loss == 1.0 and a.yuv_msssim == 50.0
    for bad, match in (("--inpanting fixed_50", "masked"), ("--host_frames", "resident"), ("--embed_inter", "resident"),
                       ("--crop_list 181_320", "even"), ("--crop_list 180_321", "even"), ("--data_path frames_dir", "no .yuv"),
                       ("--crop_list 160_320", "160"), ("--crop_list 180_160", "160"), ("--crop_list 8_12", "160")):
        for on in ("--yuv_msssim 50", "--yuv_msssim 50 --yuv_loss 1", "--yuv_msssim 50 --loss YUV420"):
            with pytest.raises(ValueError, match=match):
                mod.parse_args(f"{BASE} {on} {bad}".split())
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(ValueError, match="yuv_msssim"):
            mod.parse_args(f"{BASE} --yuv_msssim {bad}".split())
    # none of the refusals touches a run that leaves the term off, and --yuv_loss alone keeps its small crops
    a = mod.parse_args("--data_path frames_dir --crop_list 7_11 --inpanting fixed_50 --host_frames".split())
    assert a.yuv_msssim == 0
    assert mod.parse_args("--data_path clip_12x8_8bit.yuv --crop_list 8_12 --yuv_loss 1".split()).yuv_loss == 1.0


def test_refusals_when_the_record_is_made(tmp_path):
    """What only the file can tell is refused by make_term, before training starts and without a GPU."""
    from boosting_nerv_amd import yuvloss
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    gen = np.random.default_rng(6)
    path = tmp_path / "clip_16x12_8bit.yuv"
    yuvio.write(path, [tuple(p[0] for p in _planes(gen, 1, 12, 16, 8)) for _ in range(2)], "yuv420p")
    args = SimpleNamespace(data_path=str(path), crop_list="10_16", yuv_loss=0.0, yuv_msssim=50.0, yuv_loss_weights="6_1_1", loss="Fusion10_freq")
    with pytest.raises(ValueError, match="even"):
        yuvloss.make_term(args, VideoDataSet(args), "cpu", True)
    args.crop_list = "8_12"
    with pytest.raises(ValueError, match="resident"):
        yuvloss.make_term(args, VideoDataSet(args), "cpu", False)
    args.yuv_msssim = 0.0
    assert yuvloss.make_term(args, VideoDataSet(args), "cpu", False) is None


def test_the_term_record_takes_lam_ms():
    from boosting_nerv_amd import yuvloss
    from boosting_nerv_amd.engine import YuvTerm
    c = yuvio.coefficients()
    with pytest.raises(ValueError, match="lam"):                        # as before: both factors at their old values
        YuvTerm(None, c, (8, 12), (0, 0), lam=0.0)
    with pytest.raises(ValueError, match="lam"):
        YuvTerm(None, c, (8, 12), (0, 0), lam=0.0, lam_ms=0.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam_ms"):
            YuvTerm(None, c, (8, 12), (0, 0), lam_ms=bad)
    with pytest.raises(ValueError, match="lam"):
        YuvTerm(None, c, (8, 12), (0, 0), lam=-1.0, lam_ms=2.0)
    old = YuvTerm(None, c, (200, 400), (2, 4), lam=0.5)
    assert old.lam_ms == 0.0 and "MS-SSIM" not in yuvloss.describe(old)
    old.check_frame(6, 8)                                               # no 160 limit without the term
    t = YuvTerm(None, c, (200, 400), (2, 4), lam=0.0, lam_ms=50.0)
    assert t.lam == 0.0 and t.lam_ms == 50.0 and not t.pure
    assert "MS-SSIM-Y lambda 50" in yuvloss.describe(t) and yuvloss.describe(t).startswith("YUV loss: lambda 0,")
    for hw in ((160, 320), (180, 160), (6, 8)):
        with pytest.raises(ValueError, match="160"):
            t.check_frame(*hw)
    t.check_frame(162, 164)
    with pytest.raises(ValueError, match="leaves"):
        t.check_frame(200, 400)
    assert yuvloss.train_text(old, None) == ""
