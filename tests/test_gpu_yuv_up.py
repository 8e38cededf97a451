"""The plane loss through the up-sampler on the GPU (``-m gpu``): bnerv_yuv420_up_loss_fwd / _bwd behind
ops.yuv420_up_loss_value_grad_stats / ops.yuv420_up_loss against the float64 restatement yuvio.plane_loss_up_reference, the modes (accumulate,
frame selection, unaligned operands), the three step forms and the two command lines.  Fixtures are seeded (tests/yuv_up_cases.py) or the
synthetic clip; nothing is committed.

Bounds: DESIGN 33.4's, kept -- L[b] and mse_p[b] 1e-5 relative, the gradient rtol 1e-5 with atol 1e-5 max|reference gradient|.  The fp32 chain
already defined (resize_reference(clamp=False) -> plane_loss_reference -> fp32 transposed tables) differs from the float64 composition by at
most 4e-8 / 5e-8 / 8e-7 of max|grad| over these cases: one to two orders inside.  Every comparison prints its measured maximum before it asserts."""
import numpy as np
import pytest
import torch

import yuv_up_cases as K
from boosting_nerv_amd import yuvio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_dev = {}


def _case(*key, **kw):
    """K.problem with the prediction and the raw bytes on the device (uploaded once)."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _dev:
        c, P, raw, stride, ref, _ = K.problem(*key, **kw)
        _dev[k] = (c, torch.from_numpy(P.copy()).to(DEV), torch.from_numpy(raw.copy()).to(DEV), stride, ref)
    return _dev[k]


def _np(t):
    return None if t is None else t.double().cpu().numpy()


def _check(tag, loss, stats, grad, ref, lam=1.0):
    K.check(tag, float(loss), _np(stats), _np(grad), ref, lam)


def _run(case, size, window=(0, 0), src_hw=None, **kw):
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = case
    return ops.yuv420_up_loss_value_grad_stats(pred, size, raw, c, src_hw or size, window, frame_stride_bytes=stride, **kw)


# ---------------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fmt", K.FORMATS, ids=K.fmt_id)
@pytest.mark.parametrize("shape", K.CASES, ids=K.case_id)
def test_loss_stats_and_gradient_equal_the_restatement(shape, fmt):
    B, h, w, H, W = shape
    case = _case(*shape, *fmt)
    loss, stats, grad = _run(case, (H, W))
    assert loss.shape == () and tuple(stats.shape) == (B, 4) and grad.shape == case[1].shape
    _check(f"{K.case_id(shape)} {fmt}", loss, stats, grad, case[4])


@pytest.mark.parametrize("depth", [8, 10])
def test_identity_size_agrees_with_the_full_size_op(depth):
    from boosting_nerv_amd import ops
    B, h, w, H, W = K.IDENTITY
    case = _case(*K.IDENTITY, depth)
    c, pred, raw, stride, ref = case
    up = _run(case, (H, W))
    full = ops.yuv420_loss_value_grad_stats(pred, raw, c, (H, W), (0, 0))
    _check("identity: up", *up, ref)
    _check("identity: full", *full, ref)
    _check("identity: up against full", up[0], up[1], up[2], (_np(full[1])[:, 0], _np(full[1])[:, 1:], _np(full[2])))


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("window", [(2, 4), (6, 2)])
def test_windows_at_even_offsets_of_a_larger_source(window, depth):
    case = _case(1, 9, 17, 18, 34, depth, src_hw=(30, 44), window=window)
    _check(f"window {window} {depth} bit", *_run(case, (18, 34), window=window, src_hw=(30, 44)), case[4])


@pytest.mark.parametrize("depth", [8, 10])
def test_a_frame_stride_that_breaks_every_alignment(depth):
    case = _case(3, 9, 17, 18, 34, depth, stride_pad=1 if depth == 8 else 2)
    assert case[3] % 4 != 0
    _check(f"stride {case[3]}", *_run(case, (18, 34)), case[4])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("shape", [(1, 9, 17, 18, 34), (3, 9, 17, 18, 34), (1, 20, 68, 40, 136)], ids=K.case_id)
def test_unaligned_views_give_the_bits_of_the_aligned_call(shape, depth):
    """pred and grad 4 bytes off a 16-byte boundary and src one sample off: the element-by-element forms compute what the wide ones do."""
    from boosting_nerv_amd import ops
    B, h, w, H, W = shape
    c, pred, raw, stride, ref = _case(*shape, depth)
    n = pred.numel()

    def call(off_f, off_s):
        p = torch.zeros(n + 8, dtype=torch.float32, device=DEV)[off_f:off_f + n].view(B, 3, h, w).copy_(pred)
        g = torch.zeros(n + 8, dtype=torch.float32, device=DEV)[off_f:off_f + n].view(B, 3, h, w)
        s = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)[off_s:off_s + raw.numel()].copy_(raw)
        assert p.data_ptr() % 16 == 4 * off_f and g.data_ptr() % 16 == 4 * off_f and s.data_ptr() % 16 == off_s
        loss = torch.zeros((), dtype=torch.float32, device=DEV)
        return ops.yuv420_up_loss_value_grad_stats(p, (H, W), s, c, (H, W), (0, 0), grad=g, loss=loss, frame_stride_bytes=stride)
    a = call(0, 0)
    b = call(1, c.bytes_per_sample)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _check("unaligned", *b, ref)


def test_frame_sel_picks_the_frames():
    from boosting_nerv_amd import ops
    order = [2, 0, 1]
    c, pred, raw, stride, ref = _case(3, 9, 17, 18, 34, 8, n_frames=3, order=tuple(order))
    sel = torch.tensor(order, dtype=torch.float32, device=DEV)
    loss, stats, grad = ops.yuv420_up_loss_value_grad_stats(pred, (18, 34), raw, c, (18, 34), (0, 0), frame_sel=sel)
    _check("frame_sel", loss, stats, grad, ref)
    for b, k in enumerate(order):
        one = ops.yuv420_up_loss_value_grad_stats(pred[b:b + 1].contiguous(), (18, 34), raw[k * stride:(k + 1) * stride], c, (18, 34), (0, 0))
        assert torch.equal(one[1][0], stats[b])                                    # the same partial sums in the same order
        via_sel = ops.yuv420_up_loss_value_grad_stats(pred[b:b + 1].contiguous(), (18, 34), raw, c, (18, 34), (0, 0), frame_sel=sel[b:b + 1])
        assert all(torch.equal(x, y) for x, y in zip(one, via_sel))
    # a number outside the clip is clamped to its ends, never followed
    far = ops.yuv420_up_loss_value_grad_stats(pred[:1].contiguous(), (18, 34), raw, c, (18, 34), (0, 0), frame_sel=torch.tensor([99.0], device=DEV))
    last = ops.yuv420_up_loss_value_grad_stats(pred[:1].contiguous(), (18, 34), raw, c, (18, 34), (0, 0), frame_sel=torch.tensor([2.0], device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(far, last))


# ---------------------------------------------------------------------------------------------------------------------- modes
@pytest.mark.parametrize("shape", [(1, 9, 17, 18, 34), (3, 9, 17, 18, 34)], ids=K.case_id)
def test_accumulate_adds_lambda_times_the_term(shape):
    B, h, w, H, W = shape
    lam = 0.375
    case = _case(*shape)
    loss1, stats1, grad1 = _run(case, (H, W))
    gen = torch.Generator(device=DEV).manual_seed(4)
    pre_g = (torch.rand(case[1].shape, generator=gen, device=DEV) - 0.5) * 2e-3
    pre_l = torch.tensor(0.8125, device=DEV)
    g, l = pre_g.clone(), pre_l.clone()
    loss, stats, grad = _run(case, (H, W), lam=lam, grad=g, loss=l)
    assert grad is g and loss is l and torch.equal(stats, stats1)
    want_g, want_l = pre_g.double() + lam * grad1.double(), pre_l.double() + lam * loss1.double()
    bound_g = 2.0 ** -22 * (pre_g.double().abs() + (lam * grad1.double()).abs())
    err = (g.double() - want_g).abs()
    print(f"accumulate: max err / bound {float((err / bound_g.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound_g).all())
    assert abs(float(l.double() - want_l)) <= 2.0 ** -22 * (float(pre_l) + lam * float(loss1))
    # lambda on the writing call scales what is written; the stats never carry it
    loss_s, stats_s, grad_s = _run(case, (H, W), lam=lam)
    assert torch.equal(stats_s, stats1) and torch.equal(grad_s, lam * grad1) and torch.equal(loss_s, lam * loss1)
    # value and stats only: the bits of the gradient call
    loss_v, stats_v, grad_v = _run(case, (H, W), need_grad=False)
    assert grad_v is None and torch.equal(loss_v, loss1) and torch.equal(stats_v, stats1)
    l2 = pre_l.clone()
    loss_a, stats_a, grad_a = _run(case, (H, W), lam=lam, loss=l2)
    assert grad_a is None and loss_a is l2 and torch.equal(l2, l) and torch.equal(stats_a, stats1)


def test_two_calls_give_the_same_bits():
    case = _case(1, 32, 65, 64, 130, 10)
    a, b = _run(case, (64, 130)), _run(case, (64, 130))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_autograd_form_leaves_the_gradient_of_the_plain_form():
    from boosting_nerv_amd import ops
    case = _case(3, 9, 17, 18, 34)
    c, pred, raw, stride, ref = case
    loss1, stats1, grad1 = _run(case, (18, 34))
    p = pred.clone().requires_grad_(True)
    loss, stats = ops.yuv420_up_loss(p, (18, 34), raw, c, (18, 34), (0, 0))
    assert loss.requires_grad and not stats.requires_grad and torch.equal(loss.detach(), loss1) and torch.equal(stats, stats1)
    loss.backward()
    assert torch.equal(p.grad, grad1)
    p.grad = None
    (0.25 * ops.yuv420_up_loss(p, (18, 34), raw, c, (18, 34), (0, 0), weights=(6, 1, 1))[0]).backward()
    assert torch.equal(p.grad, 0.25 * grad1)
    with torch.no_grad():
        assert torch.equal(ops.yuv420_up_loss(pred, (18, 34), raw, c, (18, 34), (0, 0))[0], loss1)


def test_other_weights_reweight_the_planes():
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = _case(1, 9, 17, 18, 34)
    _, stats, grad = ops.yuv420_up_loss_value_grad_stats(pred, (18, 34), raw, c, (18, 34), (0, 0), weights=(1, 0, 3))
    _, base, _ = ops.yuv420_up_loss_value_grad_stats(pred, (18, 34), raw, c, (18, 34), (0, 0))
    assert torch.equal(stats[:, 1:], base[:, 1:])
    torch.testing.assert_close(stats[:, 0], 0.25 * base[:, 1] + 0.75 * base[:, 3], rtol=1e-6, atol=0)
    c2, P, raw_np, _, _, planes = K.problem(1, 9, 17, 18, 34)
    ref = yuvio.plane_loss_up_reference(P.astype(np.float64), planes, c2, (18, 34), (0, 0), (1, 0, 3))
    _check("weights 1_0_3", ref[0].mean(), stats, grad, ref)


def test_ops_refuse_before_any_launch():
    """Every refusal is a ValueError raised by the host, with the output tensors untouched."""
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = _case(1, 9, 17, 18, 34)
    f = ops.yuv420_up_loss_value_grad_stats
    for size in ((17, 34), (18, 33)):
        with pytest.raises(ValueError, match="even"):
            f(pred, size, raw, c, (18, 34), (0, 0))
    with pytest.raises(ValueError, match="even"):
        f(pred, (18, 34), raw, c, (18, 34), (1, 0))
    for window in ((2, 0), (0, 2)):
        with pytest.raises(ValueError, match="leaves"):
            f(pred, (18, 34), raw, c, (18, 34), window)
    with pytest.raises(ValueError, match="do not fit"):
        f(pred, (18, 34), raw[:-1], c, (18, 34), (0, 0))
    with pytest.raises(ValueError, match="frame_sel"):
        f(pred, (18, 34), raw, c, (18, 34), (0, 0), frame_sel=torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="loss to accumulate"):
        f(pred, (18, 34), raw, c, (18, 34), (0, 0), grad=torch.zeros_like(pred))
    sentinel = torch.full((), 7.0, device=DEV)
    with pytest.raises(ValueError, match="grad must be"):
        f(pred, (18, 34), raw, c, (18, 34), (0, 0), grad=torch.zeros(1, 3, 18, 34, device=DEV), loss=sentinel)
    with pytest.raises(ValueError, match="loss must be"):
        f(pred, (18, 34), raw, c, (18, 34), (0, 0), loss=torch.zeros(2, device=DEV))
    # either table over its tap limit: the forward one (1080 rows -> 18) and the adjoint one (2 columns -> 130)
    tall = torch.zeros(1, 3, 1080, 2, device=DEV)
    big = torch.zeros(130 * 18 * 3 // 2, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="taps per output"):
        f(tall, (18, 34), raw, c, (18, 34), (0, 0), loss=sentinel)
    with pytest.raises(ValueError, match="taps per input"):
        f(torch.zeros(1, 3, 9, 2, device=DEV), (18, 130), big, c, (18, 130), (0, 0), loss=sentinel, grad=torch.zeros(1, 3, 9, 2, device=DEV))
    torch.cuda.synchronize()
    assert float(sentinel) == 7.0


# ---------------------------------------------------------------------------------------------------------------------- the step
MASTER, SMALL = (270, 480), (180, 320)
_clip_cache = {}


def _clip():
    """Four frames of the synthetic clip at 480x270 stored as a raw 8-bit master and loaded back both ways:
    (YuvFile, fp32 clip resized to 180x320, raw bytes, norms, coeffs)."""
    if "clip" not in _clip_cache:
        import tempfile
        from boosting_nerv_amd import synth
        c = yuvio.coefficients("bt709", "limited", 8)
        video = synth.SyntheticVideo(4, *MASTER)
        d = tempfile.mkdtemp()
        path = f"{d}/clip_480x270_8bit.yuv"
        yuvio.write(path, [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)], c.pix_fmt)
        f = yuvio.YuvFile(path)
        raw = f.raw_to_device(DEV)
        norms = torch.tensor([(i + 1) / 4 for i in range(4)], dtype=torch.float64, device=DEV)
        _clip_cache["clip"] = (f, f.to_device(DEV, resize=SMALL), raw, norms, c)
        assert tuple(_clip_cache["clip"][1].shape) == (4, 3) + SMALL
    return _clip_cache["clip"]


def _make_step(pure, lam, **kw):
    from oracle import configs
    from boosting_nerv_amd.engine import TrainStep, YuvTerm
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    from boosting_nerv_amd.optimizer import Adan
    f, frames, raw, norms, c = _clip()
    torch.manual_seed(1)
    model = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
    opt = Adan(model.parameters(), lr=0.003)
    term = YuvTerm(raw, c, MASTER, (0, 0), weights=(6, 1, 1), lam=lam, pure=pure, up=MASTER)
    return model, TrainStep(model, opt, "YUV420" if pure else "Fusion10_freq", False, (1, 3) + SMALL, torch.device(DEV), yuv=term, **kw)


ORDER = [2, 0, 3]


def _trajectory(pure, lam, bound, **kw):
    f, frames, raw, norms, c = _clip()
    model, step = _make_step(pure, lam, **kw)
    if bound:
        step.bind_clip(frames, norms)
    losses, psnrs, stats = [], [], []
    for k in ORDER:
        if bound:
            loss, psnr = step.step_frame(k)
        else:
            loss, psnr = step(frames[k:k + 1], norms[k:k + 1], frame_idx=torch.tensor([k], device=DEV))
        losses.append(loss.clone()); psnrs.append(psnr.clone()); stats.append(step.yuv_stats_out.clone())
    return step, losses, psnrs, stats, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("bound", [False, True], ids=["call", "bound_clip"])
@pytest.mark.parametrize("pure", [False, True], ids=["added", "pure"])
def test_step_with_the_term_eager_and_replayed_agree_and_match_the_restatement(pure, bound):
    from boosting_nerv_amd import hnerv_utils as hu
    lam = 2.0
    f, frames, raw, norms, c = _clip()
    e_step, e_l, e_p, e_s, e_w = _trajectory(pure, lam, bound, use_graph=False)
    g_step, g_l, g_p, g_s, g_w = _trajectory(pure, lam, bound, use_graph=True, warmup_eager=1)
    assert e_step.graph_a is None and g_step.graph_a is not None
    for a, b in zip(e_l + e_p + e_s + e_w, g_l + g_p + g_s + g_w):
        assert torch.equal(a, b)
    # the first step's loss: the RGB loss plus lam * L_up of the restatement on the first prediction
    model, _ = _make_step(pure, lam, use_graph=False)
    k = ORDER[0]
    with torch.no_grad():
        img = model(norms[k:k + 1], norm_idx=norms[k:k + 1])[0]
        rgb = 0.0 if pure else float(hu.loss_fn(img, frames[k:k + 1], "Fusion10_freq"))
    assert tuple(img.shape) == (1, 3) + SMALL
    planes = tuple(np.asarray(p)[None] for p in f.planes(k))
    L, mse, _ = yuvio.plane_loss_up_reference(img.double().cpu().numpy(), planes, c, MASTER, (0, 0), (6, 1, 1))
    want = rgb + lam * L[0]
    print(f"step loss {float(e_l[0])!r}, RGB {rgb!r} + {lam} * {L[0]!r}: rel err {abs(float(e_l[0]) - want) / want:.2e}")
    assert abs(float(e_l[0]) - want) <= K.VALUE_TOL * want
    s0 = e_s[0].double().cpu().numpy()
    assert abs(s0[0, 0] - L[0]) <= K.VALUE_TOL * L[0] and np.all(np.abs(s0[0, 1:] - mse[0]) <= K.VALUE_TOL * mse[0])


def test_step_tests_the_window_not_the_prediction():
    from boosting_nerv_amd.engine import TrainStep, YuvTerm
    f, frames, raw, norms, c = _clip()
    model, step = _make_step(False, 1.0, use_graph=False)
    with pytest.raises(ValueError, match="leaves"):
        TrainStep(model, step.opt, "L1", False, (1, 3) + SMALL, torch.device(DEV), yuv=YuvTerm(raw, c, MASTER, (2, 0), up=MASTER))
    with pytest.raises(ValueError, match="leaves"):                   # without up the 180x320 prediction fits the 270x480 source: with it, 272 rows do not
        TrainStep(model, step.opt, "L1", False, (1, 3) + SMALL, torch.device(DEV), yuv=YuvTerm(raw, c, MASTER, (0, 0), up=(272, 480)))


# ---------------------------------------------------------------------------------------------------------------------- command lines
NERV_LINE = ("--vid tiny --model NeRV_Boost --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 270_480 "
             "--resize_list 180_320 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 "
             "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.003 -p 1 --optim_type Adan --outf ty -e 1 --not_resume")
CEM_LINE = ("--outf ty --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin "
            "--norm none --crop_list 270_480 --resize_list 180_320 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
            "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 -e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 "
            "--not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale "
            "--quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1")


@pytest.mark.isolated
@pytest.mark.parametrize("which,extra", [("train_nerv_all", "--yuv_loss 1 --yuv_upscale"), ("train_nerv_all", "--yuv_loss 1 --yuv_upscale --optim_type Adam"),
                                         ("train_nerv_compression", "--yuv_loss 1 --yuv_upscale")], ids=["all", "all_generic", "compression"])
def test_train_cli_with_and_without_the_flag(tmp_path, monkeypatch, which, extra):
    """The 4-frame tiny recipes at 180x320 from a 480x270 raw master run to the end with the term at the master's size; rank0.txt names it
    once and every train line carries the three plane PSNRs.  The same command without the flags logs neither."""
    import importlib
    from boosting_nerv_amd import synth
    mod = importlib.import_module(f"boosting_nerv_amd.{which}")
    monkeypatch.chdir(tmp_path)
    c = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(4, *MASTER)
    path = tmp_path / "clip_480x270_8bit.yuv"
    yuvio.write(path, [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)], c.pix_fmt)
    line = NERV_LINE if which == "train_nerv_all" else CEM_LINE
    log_path = tmp_path / "output" / "ty" / "tiny" / "Size0.05" / "rank0.txt"
    mod.main((line + f" --data_path {path} {extra}").split())
    log = log_path.read_text()
    assert log.count("YUV loss: lambda 1, weights 6_1_1, matrix bt709, range limited, 8 bit, at 270x480 through the up-sampler (from 180x320)") == 1
    assert "Eval at epoch 1" in log and "Resize: 270x480 -> 180x320" in log
    train = [l for l in log.splitlines() if "pred_PSNR" in l and "Step [" in l]
    assert len(train) == 4 and all("yuv_psnr: " in l for l in train)
    for l in train:
        vals = [float(v) for v in l.split("yuv_psnr: ")[1].split()[:3]]
        assert len(vals) == 3 and all(np.isfinite(v) and v > 0 for v in vals), l
    if extra != "--yuv_loss 1 --yuv_upscale":
        return                                                                    # (the run without the flags: once per script)
    log_path.unlink()
    mod.main((line + f" --data_path {path} --overwrite").split())
    log = log_path.read_text()
    assert "YUV loss" not in log and "yuv_psnr" not in log and "Eval at epoch 1" in log and "Resize: 270x480 -> 180x320" in log
