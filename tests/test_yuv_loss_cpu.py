"""The plane loss without a GPU: yuvio.plane_loss_reference against the store restatement, against autograd and against a frame
worked out by hand; what the entry point rejects; the command-line flags and their refusals."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from boosting_nerv_amd import yuvio

SHAPES = [(2, 2), (4, 6), (18, 34)]


def _planes(gen, B, h, w, depth):
    top = 2 ** depth
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    return (gen.integers(0, top, (B, h, w)).astype(dt), gen.integers(0, top, (B, h // 2, w // 2)).astype(dt),
            gen.integers(0, top, (B, h // 2, w // 2)).astype(dt))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng_name", ["limited", "full"])
def test_pre_is_the_store_restatements_pre_exactly(hw, depth, rng_name):
    gen = np.random.default_rng(hw[0] * 100 + depth)
    c = yuvio.coefficients("bt709", rng_name, depth)
    P = gen.random((2, 3) + hw)
    planes = _planes(gen, 2, hw[0], hw[1], depth)
    _, _, _, pre = yuvio.plane_loss_reference(P, planes, c, return_pre=True)
    _, ref = yuvio.to_yuv_reference(P, c, return_pre=True)
    for a, b in zip(pre, ref):
        assert a.dtype == np.float64 and np.array_equal(a, b)


def _torch_loss(P, planes, c, window, weights):
    """The definition written with float64 torch ops: the mean over the batch of L[b]."""
    import torch
    B, _, H, W = P.shape
    top, left = window
    M, m = torch.tensor(c.to_yuv), float(c.maxcode)
    w = torch.tensor(weights, dtype=torch.float64)
    w = w / w.sum()
    src = [torch.tensor(planes[0][:, top:top + H, left:left + W].astype(np.float64))]
    src += [torch.tensor(p[:, top // 2:top // 2 + H // 2, left // 2:left // 2 + W // 2].astype(np.float64)) for p in planes[1:]]
    xe = torch.arange(0, W, 2)
    L = 0.0
    for p in range(3):
        v = M[p, 0] * P[:, 0] + M[p, 1] * P[:, 1] + M[p, 2] * P[:, 2]
        if p:
            h = (v[..., torch.clamp(xe - 1, min=0)] + 2.0 * v[..., xe] + v[..., xe + 1]) / 4.0
            v = 0.5 * (h[:, 0::2] + h[:, 1::2])
        e = (float(c.offset[p]) + float(c.denom[p]) * v - src[p]) / m
        L = L + w[p] * (e * e).mean(dim=(1, 2))
    return L


@pytest.mark.parametrize("hw", SHAPES + [(6, 10)])
@pytest.mark.parametrize("depth,matrix,rng_name", [(8, "bt709", "limited"), (10, "bt601", "full")])
def test_gradient_is_the_autograd_gradient(hw, depth, matrix, rng_name):
    import torch
    gen = np.random.default_rng(7)
    c = yuvio.coefficients(matrix, rng_name, depth)
    B, (H, W) = 2, hw
    window, weights = (2, 4), (6.0, 1.0, 1.0)
    planes = _planes(gen, B, H + 4, W + 6, depth)
    P = gen.uniform(-0.25, 1.25, (B, 3, H, W))
    L, mse, grad = yuvio.plane_loss_reference(P, planes, c, window, weights)
    Pt = torch.tensor(P, requires_grad=True)
    Lt = _torch_loss(Pt, planes, c, window, weights)
    Lt.mean().backward()
    assert np.allclose(L, Lt.detach().numpy(), rtol=1e-13, atol=0)
    assert np.allclose(L, mse @ (np.array(weights) / 8.0), rtol=1e-14, atol=0)
    ref = Pt.grad.numpy()
    assert np.abs(grad - ref).max() <= 1e-12 * np.abs(ref).max()


def test_a_two_by_two_frame_by_hand():
    """One chroma sample: h(y) = (3 v(y, 0) + v(y, 1)) / 4 (column 0 is its own left neighbour), a = o + d (h(0) + h(1)) / 2; taps 3/4 and 1/4."""
    c = yuvio.coefficients("bt709", "limited", 8)
    gen = np.random.default_rng(3)
    P = gen.random((1, 3, 2, 2))
    y, u, v = np.array([[[40, 200], [90, 17]]], np.uint8), np.array([[[100]]], np.uint8), np.array([[[180]]], np.uint8)
    L, mse, grad = yuvio.plane_loss_reference(P, (y, u, v), c, (0, 0), (6, 1, 1))
    M, o, d, m = c.to_yuv, c.offset, c.denom, 255.0
    val = np.einsum("pc,cyx->pyx", M, P[0])
    e_y = (o[0] + d[0] * val[0] - y[0]) / m
    e_c = [(o[p] + d[p] * (3 * val[p, 0, 0] + val[p, 0, 1] + 3 * val[p, 1, 0] + val[p, 1, 1]) / 8 - s) / m for p, s in ((1, 100.0), (2, 180.0))]
    assert np.allclose(mse[0], [np.mean(e_y ** 2), e_c[0] ** 2, e_c[1] ** 2], rtol=1e-14, atol=0)
    assert np.isclose(L[0], (6 * mse[0, 0] + mse[0, 1] + mse[0, 2]) / 8, rtol=1e-14)
    w = np.array([6, 1, 1]) / 8
    for ch in range(3):
        for yy in range(2):
            for xx, tap in ((0, 0.75), (1, 0.25)):
                want = 2 * w[0] * d[0] * M[0, ch] * e_y[yy, xx] / (m * 4)
                want += sum(2 * w[p] * d[p] * M[p, ch] / (m * 1) * 0.5 * tap * e_c[p - 1] for p in (1, 2))
                assert np.isclose(grad[0, ch, yy, xx], want, rtol=1e-13, atol=0), (ch, yy, xx)


@pytest.mark.parametrize("depth", [8, 10])
def test_a_perfect_prediction_has_no_loss(depth):
    c = yuvio.coefficients("bt709", "limited", depth)
    s = 2 ** (depth - 8)
    H, W = 6, 10
    planes = tuple(np.full((1, H >> k, W >> k), code * s, dtype=c.dtype) for k, code in ((0, 120), (1, 110), (1, 140)))
    P = yuvio.to_rgb_reference(planes[0][0], planes[1][0], planes[2][0], c)[None]
    assert P.min() > 0.0 and P.max() < 1.0
    L, mse, grad = yuvio.plane_loss_reference(P, planes, c)
    assert L[0] < 1e-20 and mse.max() < 1e-20 and np.abs(grad).max() < 1e-10


def test_reference_refuses_odd_windows_and_bad_weights():
    c = yuvio.coefficients()
    P, planes = np.zeros((1, 3, 2, 2)), _planes(np.random.default_rng(0), 1, 4, 4, 8)
    for window in ((1, 0), (0, 1), (4, 0), (-2, 0)):
        with pytest.raises(ValueError):
            yuvio.plane_loss_reference(P, planes, c, window)
    for weights in ((0, 0, 0), (-1, 1, 1), (1, 1), "6_1"):
        with pytest.raises(ValueError):
            yuvio.plane_loss_reference(P, planes, c, (0, 0), weights)
    assert yuvio.parse_weights("6_1_1") == (6.0, 1.0, 1.0) and yuvio.parse_weights((4, 0, 0.5)) == (4.0, 0.0, 0.5)


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_point_validates_before_any_launch():
    """Every rejected argument returns BNERV_E_ARG (-1) with a message, with no GPU in the machine."""
    from boosting_nerv_amd import _lib as L, ops
    lib = L.load()
    assert lib.bnerv_abi_version() == 9                                 # additive
    assert callable(ops.yuv420_loss) and callable(ops.yuv420_loss_value_grad_stats)
    k = yuvio.coefficients("bt709", "limited", 8).store_struct()
    kp, one = C.byref(k), C.c_void_p(64)
    w611 = (C.c_float * 3)(6, 1, 1)

    def loss(pred=one, B=1, H=2, W=2, src=one, bps=1, stride=6, n_frames=1, src_h=2, src_w=2, top=0, left=0, sel=None, coeffs=kp, weights=w611,
             grad=one, out=one, stats=one, ws=one, ws_bytes=1 << 20):
        return lib.bnerv_yuv420_loss(None, pred, B, H, W, src, bps, stride, n_frames, src_h, src_w, top, left, sel, coeffs, weights, 1.0, grad, 0, out,
                                     stats, ws, ws_bytes)

    for bad in (dict(pred=None), dict(src=None), dict(coeffs=None), dict(weights=None), dict(out=None), dict(stats=None), dict(ws=None)):
        assert loss(**bad) == -1 and b"yuv420_loss: null" in lib.bnerv_last_error(), bad
    for bad in (dict(H=3, src_h=4, stride=12), dict(W=3, src_w=4, stride=12), dict(src_h=3), dict(src_w=3)):
        assert loss(**bad) == -1 and b"even" in lib.bnerv_last_error(), bad
    big = dict(src_h=8, src_w=8, stride=96)
    for bad in (dict(top=1), dict(left=1), dict(top=-2), dict(left=-2)):
        assert loss(**big, **bad) == -1 and b"must be even" in lib.bnerv_last_error(), bad
    for bad in (dict(top=8), dict(left=8), dict(H=10), dict(W=10), dict(top=2 ** 31 - 2)):
        assert loss(**big, **bad) == -1 and b"leaves" in lib.bnerv_last_error(), bad
    assert loss(stride=5) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert loss(bps=2, stride=11) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert loss(bps=2, stride=13) == -1 and b"odd" in lib.bnerv_last_error()
    for bps in (0, 3, 4):
        assert loss(bps=bps) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    for w in ((-1, 1, 1), (1, -1, 1), (1, 1, -0.5), (0, 0, 0), (float("nan"), 1, 1)):
        assert loss(weights=(C.c_float * 3)(*w)) == -1 and b"weights" in lib.bnerv_last_error(), w
    assert loss(B=2) == -1 and b"without frame_sel" in lib.bnerv_last_error()      # two samples, one frame, no selector
    for bad in (dict(B=0), dict(B=70000, sel=one), dict(H=0), dict(W=0), dict(n_frames=0)):
        assert loss(**bad) == -1, bad
    for bad in (dict(pred=C.c_void_p(66)), dict(grad=C.c_void_p(66)), dict(sel=C.c_void_p(66))):
        assert loss(**bad) == -1 and b"4-byte" in lib.bnerv_last_error(), bad
    assert loss(ws_bytes=0) != 0 and b"workspace" in lib.bnerv_last_error()
    assert lib.bnerv_yuv420_loss_ws_bytes(1, 2, 2) == 4 * 3 * 4 and lib.bnerv_yuv420_loss_ws_bytes(3, 64, 130) == 3 * 5 * 4 * 3 * 4
    assert lib.bnerv_yuv420_loss_ws_bytes(0, 2, 2) == 0


# ---------------------------------------------------------------------------------------------------------------------- flags
BASE = "--data_path clip_12x8_8bit.yuv --crop_list 8_12"


@pytest.mark.parametrize("which", ["train_nerv_all", "train_nerv_compression"])
def test_train_parsers_take_the_flags_and_refuse_what_no_run_can_honour(which):
    import importlib
    mod = importlib.import_module(f"boosting_nerv_amd.{which}")
    a = mod.parse_args([])
    assert a.yuv_loss == 0 and a.yuv_loss_weights == "6_1_1" and a.loss != "YUV420"      # off by default
    a = mod.parse_args(f"{BASE} --yuv_loss 0.5 --yuv_loss_weights 4_1_1".split())
    assert a.yuv_loss == 0.5 and a.yuv_loss_weights == "4_1_1"
    a = mod.parse_args(f"{BASE} --loss YUV420".split())
    assert a.loss == "YUV420" and a.yuv_loss == 1.0                                      # the pure form switches the term on
    assert mod.parse_args(f"{BASE} --loss YUV420 --yuv_loss 3".split()).yuv_loss == 3.0
    for bad, match in (("--inpanting fixed_50", "masked"), ("--host_frames", "resident"), ("--embed_inter", "resident"),
                       ("--crop_list 7_12", "even"), ("--crop_list 8_11", "even"), ("--data_path frames_dir", "no .yuv"),
                       ("--yuv_loss_weights 0_0_0", "weights"), ("--yuv_loss_weights 6_1", "weights"), ("--yuv_loss_weights 6_-1_1", "weights")):
        for on in ("--yuv_loss 1", "--loss YUV420"):
            with pytest.raises(ValueError, match=match):
                mod.parse_args(f"{BASE} {on} {bad}".split())
    with pytest.raises(ValueError, match="yuv_loss"):
        mod.parse_args(f"{BASE} --yuv_loss -1".split())
    # none of the refusals touches a run that leaves the term off
    a = mod.parse_args("--data_path frames_dir --crop_list 7_11 --inpanting fixed_50 --host_frames".split())
    assert a.yuv_loss == 0


def test_an_odd_crop_offset_is_refused_before_training(tmp_path):
    """A 10-row crop of a 12-row source sits at row 1: no chroma row covers it.  Refused when the record is made, without a GPU."""
    from boosting_nerv_amd import yuvloss
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    gen = np.random.default_rng(6)
    path = tmp_path / "clip_16x12_8bit.yuv"
    yuvio.write(path, [tuple(p[0] for p in _planes(gen, 1, 12, 16, 8)) for _ in range(2)], "yuv420p")
    args = SimpleNamespace(data_path=str(path), crop_list="10_16", yuv_loss=1.0, yuv_loss_weights="6_1_1", loss="Fusion10_freq")
    with pytest.raises(ValueError, match="even"):
        yuvloss.make_term(args, VideoDataSet(args), "cpu", True)
    args.crop_list = "8_12"
    with pytest.raises(ValueError, match="resident"):
        yuvloss.make_term(args, VideoDataSet(args), "cpu", False)
    args.yuv_loss = 0.0
    assert yuvloss.make_term(args, VideoDataSet(args), "cpu", False) is None


def test_the_term_record_refuses_a_mask_and_odd_windows():
    from boosting_nerv_amd.engine import YuvTerm
    c = yuvio.coefficients()
    for window in ((1, 0), (0, 3)):
        with pytest.raises(ValueError, match="even"):
            YuvTerm(None, c, (8, 12), window)
    with pytest.raises(ValueError, match="lam"):
        YuvTerm(None, c, (8, 12), (0, 0), lam=0.0)
    t = YuvTerm(None, c, (8, 12), (2, 4), weights="6_1_1", lam=0.5)
    assert t.weights == (6.0, 1.0, 1.0) and t.lam == 0.5 and not t.pure
    with pytest.raises(ValueError, match="even"):
        t.check_frame(5, 8)
    with pytest.raises(ValueError, match="leaves"):
        t.check_frame(8, 8)
    t.check_frame(6, 8)
