"""The plane loss on the GPU (``-m gpu``): bnerv_yuv420_loss behind ops.yuv420_loss_value_grad_stats / ops.yuv420_loss against
the float64 restatement yuvio.plane_loss_reference, its modes (accumulate, frame selection, unaligned operands), the three step forms and the two
command lines.  Fixtures are seeded random samples or the synthetic clip; nothing is committed.

Bounds (the issue's, from the arithmetic): the loss is a plain quadratic with every intermediate at or below about 1 in magnitude; an error e_p
carries a handful of fp32 roundings (about 5e-7 absolute), the sums add non-negative terms in a fixed order.  L[b] and mse_p[b]: 1e-5 relative;
the gradient: rtol 1e-5 with atol 1e-5 max|reference gradient|.  Every comparison prints its measured maximum before it asserts."""
import numpy as np
import pytest
import torch

from boosting_nerv_amd import yuvio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_TOL = 1e-5

SHAPES = [(1, 2, 2), (1, 2, 4), (1, 4, 6), (1, 6, 10), (1, 18, 34), (3, 18, 34), (1, 64, 130)]
FORMATS = [(8, "bt709", "limited"), (10, "bt709", "limited"), (8, "bt601", "limited"), (10, "bt709", "full")]

_cache = {}


def _case(B, H, W, depth, matrix="bt709", rng_name="limited", src_hw=None, window=(0, 0), lo=0.0, hi=1.0, n_frames=None, order=None, stride_pad=0):
    """One seeded problem and its float64 answer, made once: (coeffs, pred fp32 [B, 3, H, W] on the device, raw device bytes, stride, reference)
    with reference = plane_loss_reference of the fp32 prediction (L [B], mse [B, 3], grad [B, 3, H, W]).  order: sample b against frame order[b]."""
    key = (B, H, W, depth, matrix, rng_name, src_hw, window, lo, hi, n_frames, None if order is None else tuple(order), stride_pad)
    if key in _cache:
        return _cache[key]
    sh, sw = src_hw or (H, W)
    n = n_frames or B
    gen = np.random.default_rng(1000 * H + W + depth + B)
    c = yuvio.coefficients(matrix, rng_name, depth)
    top = 2 ** depth
    frames = []
    for _ in range(n):
        f = [gen.integers(0, top, s).astype(c.dtype) for s in ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))]
        for p in f:
            p.reshape(-1)[0], p.reshape(-1)[-1] = top - 1, 0
        frames.append(tuple(f))
    frame_bytes = sh * sw * 3 // 2 * c.bytes_per_sample
    stride = frame_bytes + stride_pad
    raw = b"".join(b"".join(p.tobytes() for p in f) + b"\xff" * stride_pad for f in frames)
    P = gen.uniform(lo, hi, (B, 3, H, W)).astype(np.float32)
    pick = list(range(B)) if order is None else list(order)
    planes = tuple(np.stack([frames[k][p] for k in pick]) for p in range(3))
    ref = yuvio.plane_loss_reference(P.astype(np.float64), planes, c, window, (6, 1, 1))
    out = (c, torch.from_numpy(P).to(DEV), torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV), stride, ref)
    _cache[key] = out
    return out


def _check(tag, loss, stats, grad, ref, lam=1.0):
    L, mse, g = ref
    stats = stats.double().cpu().numpy()
    e_l = np.abs(stats[:, 0] - L).max() / np.abs(L).max()
    e_m = (np.abs(stats[:, 1:] - mse) / mse).max()
    e_t = abs(float(loss) - lam * L.mean()) / (lam * L.mean())
    print(f"{tag}: rel err L[b] {e_l:.2e}, mse_p {e_m:.2e}, loss {e_t:.2e}", end="")
    if grad is not None:
        got = grad.double().cpu().numpy()
        e_g = np.abs(got - lam * g).max() / (lam * np.abs(g).max())
        print(f", grad max err / max|ref| {e_g:.2e}", end="")
    print()
    assert np.all(np.abs(stats[:, 0] - L) <= VALUE_TOL * np.abs(L)) and np.all(np.abs(stats[:, 1:] - mse) <= VALUE_TOL * mse)
    assert e_t <= VALUE_TOL
    if grad is not None:
        assert np.all(np.abs(got - lam * g) <= GRAD_TOL * np.abs(lam * g) + GRAD_TOL * lam * np.abs(g).max())


def _run(case, H, W, window=(0, 0), src_hw=None, **kw):
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = case
    return ops.yuv420_loss_value_grad_stats(pred, raw, c, src_hw or (H, W), window, frame_stride_bytes=stride, **kw)


# ---------------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: f"{f[0]}bit_{f[1]}_{f[2]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_stats_and_gradient_equal_the_restatement(shape, fmt):
    B, H, W = shape
    case = _case(B, H, W, *fmt)
    loss, stats, grad = _run(case, H, W)
    assert loss.shape == () and tuple(stats.shape) == (B, 4) and grad.shape == case[1].shape
    _check(f"{shape} {fmt}", loss, stats, grad, case[4])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("window", [(2, 4), (6, 2)])
def test_windows_at_even_offsets_of_a_larger_source(window, depth):
    case = _case(1, 18, 34, depth, src_hw=(30, 44), window=window)
    _check(f"window {window} {depth} bit", *_run(case, 18, 34, window=window, src_hw=(30, 44)), case[4])


@pytest.mark.parametrize("depth", [8, 10])
def test_a_frame_stride_that_breaks_every_alignment(depth):
    """Three frames, each one sample further from the alignment of the one before it: every access picks its form per address."""
    case = _case(3, 18, 34, depth, stride_pad=1 if depth == 8 else 2)
    assert case[3] % 4 != 0
    _check(f"stride {case[3]}", *_run(case, 18, 34), case[4])


@pytest.mark.parametrize("depth", [8, 10])
def test_values_outside_the_unit_interval_are_not_clamped(depth):
    case = _case(1, 18, 34, depth, lo=-0.25, hi=1.25)
    assert float(case[1].min()) < -0.2 and float(case[1].max()) > 1.2
    _check("unclamped", *_run(case, 18, 34), case[4])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("shape", [(1, 18, 34), (3, 18, 34), (1, 64, 130)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_views_give_the_bits_of_the_aligned_call(shape, depth):
    """pred and grad 4 bytes off a 16-byte boundary and src one sample off: the element-by-element forms compute what the wide ones do."""
    from boosting_nerv_amd import ops
    B, H, W = shape
    c, pred, raw, stride, ref = _case(B, H, W, depth)
    n = pred.numel()

    def call(off_f, off_s):
        p = torch.zeros(n + 8, dtype=torch.float32, device=DEV)[off_f:off_f + n].view(B, 3, H, W).copy_(pred)
        g = torch.zeros(n + 8, dtype=torch.float32, device=DEV)[off_f:off_f + n].view(B, 3, H, W)
        s = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)[off_s:off_s + raw.numel()].copy_(raw)
        assert p.data_ptr() % 16 == 4 * off_f and g.data_ptr() % 16 == 4 * off_f and s.data_ptr() % 16 == off_s
        loss = torch.zeros((), dtype=torch.float32, device=DEV)
        return ops.yuv420_loss_value_grad_stats(p, s, c, (H, W), (0, 0), grad=g, loss=loss, frame_stride_bytes=stride)
    a = call(0, 0)
    b = call(1, c.bytes_per_sample)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _check("unaligned", *b, ref)


def test_frame_sel_picks_the_frames():
    """frame_sel = [2, 0, 1] on a 3-frame clip: the restatement on the permuted frames, and per sample the sums of three single calls."""
    from boosting_nerv_amd import ops
    order = [2, 0, 1]
    c, pred, raw, stride, ref = _case(3, 18, 34, 8, n_frames=3, order=order)
    sel = torch.tensor(order, dtype=torch.float32, device=DEV)
    loss, stats, grad = ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (0, 0), frame_sel=sel)
    _check("frame_sel", loss, stats, grad, ref)
    for b, k in enumerate(order):
        one = ops.yuv420_loss_value_grad_stats(pred[b:b + 1].contiguous(), raw[k * stride:(k + 1) * stride], c, (18, 34), (0, 0))
        assert torch.equal(one[1][0], stats[b])                                    # the same partial sums in the same order
        # (the batch mean's 1 / B is folded into the rounded gradient constants: close, not equal)
        torch.testing.assert_close(one[2][0] / 3.0, grad[b], rtol=1e-6, atol=1e-6 * float(grad[b].abs().max()))
        via_sel = ops.yuv420_loss_value_grad_stats(pred[b:b + 1].contiguous(), raw, c, (18, 34), (0, 0), frame_sel=sel[b:b + 1])
        assert all(torch.equal(x, y) for x, y in zip(one, via_sel))
    # a number outside the clip is clamped to its ends, never followed
    far = ops.yuv420_loss_value_grad_stats(pred[:1].contiguous(), raw, c, (18, 34), (0, 0), frame_sel=torch.tensor([99.0], device=DEV))
    last = ops.yuv420_loss_value_grad_stats(pred[:1].contiguous(), raw, c, (18, 34), (0, 0), frame_sel=torch.tensor([2.0], device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(far, last))


# ---------------------------------------------------------------------------------------------------------------------- modes
@pytest.mark.parametrize("shape", [(1, 18, 34), (3, 18, 34)], ids=lambda s: "x".join(map(str, s)))
def test_accumulate_adds_lambda_times_the_term(shape):
    B, H, W = shape
    lam = 0.375
    case = _case(B, H, W, 8)
    loss1, stats1, grad1 = _run(case, H, W)
    gen = torch.Generator(device=DEV).manual_seed(4)
    pre_g = (torch.rand(case[1].shape, generator=gen, device=DEV) - 0.5) * 2e-3
    pre_l = torch.tensor(0.8125, device=DEV)
    g, l = pre_g.clone(), pre_l.clone()
    loss, stats, grad = _run(case, H, W, lam=lam, grad=g, loss=l)
    assert grad is g and loss is l and torch.equal(stats, stats1)
    want_g, want_l = pre_g.double() + lam * grad1.double(), pre_l.double() + lam * loss1.double()
    bound_g = 2.0 ** -22 * (pre_g.double().abs() + (lam * grad1.double()).abs())
    err = (g.double() - want_g).abs()
    print(f"accumulate: max err / bound {float((err / bound_g.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound_g).all())
    assert abs(float(l.double() - want_l)) <= 2.0 ** -22 * (float(pre_l) + lam * float(loss1))
    # lambda on the writing call scales what is written; the stats never carry it
    loss_s, stats_s, grad_s = _run(case, H, W, lam=lam)
    assert torch.equal(stats_s, stats1) and torch.equal(grad_s, lam * grad1) and torch.equal(loss_s, lam * loss1)
    # value and stats only
    loss_v, stats_v, grad_v = _run(case, H, W, need_grad=False)
    assert grad_v is None and torch.equal(loss_v, loss1) and torch.equal(stats_v, stats1)
    l2 = pre_l.clone()
    loss_a, stats_a, grad_a = _run(case, H, W, lam=lam, loss=l2)
    assert grad_a is None and loss_a is l2 and torch.equal(l2, l) and torch.equal(stats_a, stats1)


def test_two_calls_give_the_same_bits():
    case = _case(1, 64, 130, 10)
    a, b = _run(case, 64, 130), _run(case, 64, 130)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_autograd_form_leaves_the_gradient_of_the_plain_form():
    from boosting_nerv_amd import ops
    c, pred, raw, stride, ref = _case(3, 18, 34, 8)
    loss1, stats1, grad1 = _run((c, pred, raw, stride, ref), 18, 34)
    p = pred.clone().requires_grad_(True)
    loss, stats = ops.yuv420_loss(p, raw, c, (18, 34), (0, 0))
    assert loss.requires_grad and not stats.requires_grad and torch.equal(loss.detach(), loss1) and torch.equal(stats, stats1)
    loss.backward()
    assert torch.equal(p.grad, grad1)
    p.grad = None
    (0.25 * ops.yuv420_loss(p, raw, c, (18, 34), (0, 0), weights=(6, 1, 1))[0]).backward()
    assert torch.equal(p.grad, 0.25 * grad1)
    with torch.no_grad():
        assert torch.equal(ops.yuv420_loss(pred, raw, c, (18, 34), (0, 0))[0], loss1)


def test_other_weights_reweight_the_planes():
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = _case(1, 18, 34, 8)
    _, stats, _ = ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (0, 0), weights=(1, 0, 3))
    _, base, _ = ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (0, 0))
    assert torch.equal(stats[:, 1:], base[:, 1:])
    torch.testing.assert_close(stats[:, 0], 0.25 * base[:, 1] + 0.75 * base[:, 3], rtol=1e-6, atol=0)


def test_ops_refuse_what_the_kernel_must_not_see():
    from boosting_nerv_amd import ops
    c, pred, raw, stride, _ = _case(1, 18, 34, 8)
    with pytest.raises(ValueError, match="do not fit"):
        ops.yuv420_loss_value_grad_stats(pred, raw[:-1], c, (18, 34), (0, 0))
    with pytest.raises(ValueError, match="frame_sel"):
        ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (0, 0), frame_sel=torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="loss to accumulate"):
        ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (0, 0), grad=torch.zeros_like(pred))
    with pytest.raises(Exception, match="even"):
        ops.yuv420_loss_value_grad_stats(pred, raw, c, (18, 34), (1, 0))


# ---------------------------------------------------------------------------------------------------------------------- the step
def _clip(tmp_path_factory=None):
    """Four frames of the synthetic clip stored as a raw 8-bit file and loaded back both ways: (YuvFile, fp32 clip, raw bytes, norms, coeffs)."""
    if "clip" not in _cache:
        import tempfile
        from boosting_nerv_amd import synth
        c = yuvio.coefficients("bt709", "limited", 8)
        video = synth.SyntheticVideo(4, 180, 320)
        d = tempfile.mkdtemp()
        path = f"{d}/clip_320x180_8bit.yuv"
        yuvio.write(path, [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)], c.pix_fmt)
        f = yuvio.YuvFile(path)
        raw = f.raw_to_device(DEV, chunk=3)                                        # (two chunks: both pinned buffers)
        assert raw.dtype == torch.uint8 and np.array_equal(raw.cpu().numpy(), np.asarray(f.raw(0, 4)))
        assert torch.equal(f.raw_to_device(DEV, count=2), raw[:2 * f.frame_bytes])
        norms = torch.tensor([(i + 1) / 4 for i in range(4)], dtype=torch.float64, device=DEV)
        _cache["clip"] = (f, f.to_device(DEV), raw, norms, c)
    return _cache["clip"]


def _make_step(pure, lam, **kw):
    from oracle import configs
    from boosting_nerv_amd.engine import TrainStep, YuvTerm
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    from boosting_nerv_amd.optimizer import Adan
    f, frames, raw, norms, c = _clip()
    torch.manual_seed(1)
    model = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
    opt = Adan(model.parameters(), lr=0.003)
    term = YuvTerm(raw, c, (180, 320), (0, 0), weights=(6, 1, 1), lam=lam, pure=pure)
    return model, TrainStep(model, opt, "YUV420" if pure else "Fusion10_freq", False, (1, 3, 180, 320), torch.device(DEV), yuv=term, **kw)


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
    from boosting_nerv_amd import hnerv_utils as hu, ops
    lam = 2.0
    f, frames, raw, norms, c = _clip()
    e_step, e_l, e_p, e_s, e_w = _trajectory(pure, lam, bound, use_graph=False)
    g_step, g_l, g_p, g_s, g_w = _trajectory(pure, lam, bound, use_graph=True, warmup_eager=1)
    assert e_step.graph_a is None and g_step.graph_a is not None
    for a, b in zip(e_l + e_p + e_s + e_w, g_l + g_p + g_s + g_w):
        assert torch.equal(a, b)
    # the first step's loss: the RGB loss plus lam * L of the restatement on the first prediction
    model, _ = _make_step(pure, lam, use_graph=False)
    k = ORDER[0]
    with torch.no_grad():
        img = model(norms[k:k + 1], norm_idx=norms[k:k + 1])[0]
        rgb = 0.0 if pure else float(hu.loss_fn(img, frames[k:k + 1], "Fusion10_freq"))
    planes = tuple(np.asarray(p)[None] for p in f.planes(k))
    L, mse, _ = yuvio.plane_loss_reference(img.double().cpu().numpy(), planes, c, (0, 0), (6, 1, 1))
    want = rgb + lam * L[0]
    print(f"step loss {float(e_l[0])!r}, RGB {rgb!r} + {lam} * {L[0]!r}: rel err {abs(float(e_l[0]) - want) / want:.2e}")
    assert abs(float(e_l[0]) - want) <= VALUE_TOL * want
    s0 = e_s[0].double().cpu().numpy()
    assert abs(s0[0, 0] - L[0]) <= VALUE_TOL * L[0] and np.all(np.abs(s0[0, 1:] - mse[0]) <= VALUE_TOL * mse[0])
    torch.testing.assert_close(e_p[0], ops.psnr(img, frames[k:k + 1]), rtol=1e-5, atol=0)      # psnr_out stays the RGB PSNR in both forms
    # and the term is in the trajectory: the step without it takes another one
    if not pure:
        from oracle import configs
        from boosting_nerv_amd.engine import TrainStep
        from boosting_nerv_amd.model_nerv import NeRV_Boost
        from boosting_nerv_amd.optimizer import Adan
        torch.manual_seed(1)
        m0 = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
        plain = TrainStep(m0, Adan(m0.parameters(), lr=0.003), "Fusion10_freq", False, (1, 3, 180, 320), torch.device(DEV), use_graph=False)
        l0, _ = plain(frames[k:k + 1], norms[k:k + 1])
        assert plain.yuv_stats_out is None and abs(float(l0) - rgb) <= 1e-6 * rgb and float(e_l[0]) > float(l0)


def test_step_refuses_a_mask_an_odd_crop_and_a_missing_frame_number():
    from boosting_nerv_amd.engine import YuvTerm
    f, frames, raw, norms, c = _clip()
    model, step = _make_step(False, 1.0, use_graph=False)
    with pytest.raises(ValueError, match="frame_idx"):
        step(frames[:1], norms[:1])
    from boosting_nerv_amd.engine import TrainStep
    term = YuvTerm(raw, c, (180, 320), (0, 0))
    with pytest.raises(ValueError, match="mask"):
        TrainStep(model, step.opt, "L1", False, (1, 3, 180, 320), torch.device(DEV), yuv=term, mask=torch.ones(180, 320))
    with pytest.raises(ValueError, match="leaves"):
        TrainStep(model, step.opt, "L1", False, (1, 3, 180, 322), torch.device(DEV), yuv=term)


# ---------------------------------------------------------------------------------------------------------------------- command lines
NERV_LINE = ("--vid tiny --model NeRV_Boost --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 "
             "--resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 "
             "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.003 -p 1 --optim_type Adan --outf ty -e 1 --not_resume")
CEM_LINE = ("--outf ty --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin "
            "--norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
            "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 -e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 "
            "--not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale "
            "--quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1")


@pytest.mark.isolated
@pytest.mark.parametrize("which,extra", [("train_nerv_all", "--yuv_loss 1"), ("train_nerv_all", "--loss YUV420"), ("train_nerv_all", "--yuv_loss 1 --optim_type Adam"),
                                         ("train_nerv_compression", "--yuv_loss 1")], ids=["all", "all_pure", "all_generic", "compression"])
def test_train_cli_with_and_without_the_term(tmp_path, monkeypatch, which, extra):
    """The 4-frame tiny recipes on the synthetic clip stored as a raw file run to the end with the term; rank0.txt names it once and every
    train line carries the three plane PSNRs.  The same command without the flag logs neither."""
    import importlib
    from boosting_nerv_amd import synth
    mod = importlib.import_module(f"boosting_nerv_amd.{which}")
    monkeypatch.chdir(tmp_path)
    c = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(4, 180, 320)
    path = tmp_path / "clip_320x180_8bit.yuv"
    yuvio.write(path, [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)], c.pix_fmt)
    line = NERV_LINE if which == "train_nerv_all" else CEM_LINE
    log_path = tmp_path / "output" / "ty" / "tiny" / "Size0.05" / "rank0.txt"
    mod.main((line + f" --data_path {path} {extra}").split())
    log = log_path.read_text()
    assert log.count("YUV loss: lambda 1, weights 6_1_1, matrix bt709, range limited") == 1 and "Eval at epoch 1" in log
    assert ("pure" in log) == ("YUV420" in extra)
    train = [l for l in log.splitlines() if "pred_PSNR" in l and "Step [" in l]
    assert len(train) == 4 and all("yuv_psnr: " in l for l in train)
    for l in train:
        vals = [float(v) for v in l.split("yuv_psnr: ")[1].split()[:3]]
        assert len(vals) == 3 and all(np.isfinite(v) and v > 0 for v in vals), l
    if extra != "--yuv_loss 1":
        return                                                                    # (the run without the flag: once per script)
    log_path.unlink()
    mod.main((line + f" --data_path {path} --overwrite " + extra.replace("--yuv_loss 1", "").replace("--loss YUV420", "")).split())
    log = log_path.read_text()
    assert "YUV loss" not in log and "yuv_psnr" not in log and "Eval at epoch 1" in log
