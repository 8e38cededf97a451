"""GPU tests (``-m gpu``) of the single-scale SSIM losses -- SSIM, Fusion1-9, L1_ssim_freq (csrc/loss.hip: ssim_head / ssim_tail, entry
bnerv_loss_ssim_fwd_bwd) -- and of ops.ssim: value and gradient against the goldens of the reference's loss_fn
(tests/golden/loss_ssim.npz, tools/make_ssim_loss_goldens.py) and against float64 autograd over oracle.msssim_ref.ssim, the statistics
columns, the fused and value-only forms, full-size frames, the captured train step and the train scripts' CLI.

Tolerances are the project's own (test_gpu_ops.test_loss_against_goldens_and_oracle): value 2e-4 relative, gradient rtol 2e-3 with
atol 2e-3 max|ref|; end PSNR of a short schedule within 0.02 dB of a stock-ops restatement (test_gpu_hnerv)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hnerv_ref
from conftest import group, load_golden
from oracle import cpu_ref, msssim_ref
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TYPES = ("SSIM", "Fusion1", "Fusion2", "Fusion3", "Fusion4", "Fusion5", "Fusion6", "Fusion7", "Fusion8", "Fusion9", "L1_ssim_freq")
SSIM_TYPES = tuple(t for t in TYPES if t not in ("Fusion7", "Fusion8"))
COEFFS = {            # (c_l1, c_l2, c_ss, c_fft): the issue's table, restated here so that the test does not read the table it checks
    "SSIM": (0, 0, 1, 0), "Fusion1": (0, .3, .7, 0), "Fusion2": (.3, 0, .7, 0), "Fusion3": (0, .5, .5, 0), "Fusion4": (.5, 0, .5, 0),
    "Fusion5": (0, .7, .3, 0), "Fusion6": (.7, 0, .3, 0), "Fusion7": (.3, .7, 0, 0), "Fusion8": (.5, .5, 0, 0), "Fusion9": (.9, 0, .1, 0),
    "L1_ssim_freq": (42, 0, 18, 1),
}


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


def _inputs(tag):
    npz = load_golden("loss_ssim.npz")
    src = load_golden("loss.npz") if str(npz[f"{tag}/inputs"]) == "loss.npz" else npz
    return npz, torch.from_numpy(src[f"{tag}/pred"]).clone(), torch.from_numpy(src[f"{tag}/target"])


def _seeded(npz, tag):
    g = torch.Generator().manual_seed(int(npz[f"{tag}/seed"]))
    shape = tuple(int(v) for v in npz[f"{tag}/shape"])
    tgt = torch.rand(shape, generator=g)
    return (tgt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), tgt


def loss_f64(pred, tgt, lt):
    """The loss from its definition in float64: plain torch ops and msssim_ref.ssim."""
    c1, c2, cs, cf = COEFFS[lt]
    d = pred - tgt
    loss = torch.zeros(pred.shape[0], dtype=pred.dtype)
    if c1:
        loss = loss + c1 * d.abs().flatten(1).mean(1)
    if c2:
        loss = loss + c2 * (d * d).flatten(1).mean(1)
    if cs:
        loss = loss + cs * (1 - msssim_ref.ssim(pred, tgt, data_range=1, size_average=False))
    if cf:
        loss = loss + cf * torch.view_as_real(torch.fft.fft2(pred) - torch.fft.fft2(tgt)).abs().flatten(1).mean(1)
    return loss.mean()


@pytest.mark.parametrize("tag", ["sub160", "edge", "odd", "small"])
@pytest.mark.parametrize("lt", TYPES)
def test_value_and_gradient_against_goldens_and_float64(ops, lt, tag):
    npz, pred, tgt = _inputs(tag)
    p64 = pred.double().requires_grad_(True)
    ref = loss_f64(p64, tgt.double(), lt)
    rgrad, = torch.autograd.grad(ref, [p64])
    pg = pred.to(DEV).requires_grad_(True)
    td = tgt.to(DEV)
    loss, stats = ops.loss_with_stats(pg, td, lt)
    gold = float(npz[f"{tag}/{lt}/loss"])
    ggrad, = torch.autograd.grad(loss, [pg])
    print(f"{lt} {tag}: loss {loss.item():.8f} golden {gold:.8f} f64 {ref.item():.8f}; max|grad - f64| {float((ggrad.cpu().double() - rgrad).abs().max()):.3e} "
          f"of max|grad| {float(rgrad.abs().max()):.3e}")
    assert abs(loss.item() - gold) <= 2e-4 * abs(gold), (loss.item(), gold)
    assert abs(loss.item() - ref.item()) <= 2e-4 * abs(ref.item()), (loss.item(), ref.item())
    close(ggrad, rgrad, rtol=2e-3, atol=2e-3 * float(rgrad.abs().max()), msg=f"{lt} {tag} grad vs float64")
    if f"{tag}/{lt}/grad" in npz.files:                   # the reference's own gradient, in full
        gg = torch.from_numpy(npz[f"{tag}/{lt}/grad"])
        close(ggrad, gg, rtol=2e-3, atol=2e-3 * float(gg.abs().max()), msg=f"{lt} {tag} grad vs golden")
    else:
        idx, val = torch.from_numpy(npz[f"{tag}/{lt}/grad.idx"]), torch.from_numpy(npz[f"{tag}/{lt}/grad.val"])
        close(ggrad.flatten().cpu()[idx], val, rtol=2e-3, atol=2e-3 * float(val.abs().max()), msg=f"{lt} {tag} grad samples vs golden")
    # the train step's fused form: same value, same gradient, same statistics
    l2, st2, g2 = ops.loss_value_grad_stats(pg, td, lt)
    assert l2.item() == loss.item() and torch.equal(g2, ggrad) and torch.equal(st2, stats)
    # value only (no gradient asked for): the same value and statistics
    with torch.no_grad():
        l3, st3 = ops.loss_with_stats(pg.detach(), td, lt)
    assert l3.item() == loss.item() and torch.equal(st3, stats)
    assert torch.equal(stats[:, 4], ops.psnr(pg, td))
    if lt in SSIM_TYPES:
        assert torch.equal(stats[:, 3], ops.ssim(pg, td))


@pytest.mark.parametrize("tag", ["sub160", "edge", "odd", "small"])
def test_ssim_metric_and_statistics(ops, tag):
    npz, pred, tgt = _inputs(tag)
    pg, td = pred.to(DEV), tgt.to(DEV)
    got = ops.ssim(pg, td)
    close(got, msssim_ref.ssim(pred, tgt, data_range=1, size_average=False), rtol=1e-4, atol=1e-5, msg="ssim")
    close(got, msssim_ref.ssim(pred.double(), tgt.double(), data_range=1, size_average=False), rtol=1e-4, atol=1e-5, msg="ssim vs float64")
    close(got, torch.from_numpy(npz[f"{tag}/ssim_b"]), rtol=1e-4, atol=1e-5, msg="ssim vs golden")
    for lt in ("SSIM", "Fusion6", "L1_ssim_freq"):
        _, stats = ops.loss_with_stats(pg.clone().requires_grad_(True), td, lt)
        assert torch.equal(stats[:, 3], got) and torch.equal(stats[:, 4], ops.psnr(pg, td))
        close(stats[:, 1], (pred - tgt).abs().flatten(1).sum(1), rtol=1e-5, atol=1e-3, msg="sum|d|")
        close(stats[:, 2], ((pred - tgt) ** 2).flatten(1).sum(1), rtol=1e-5, atol=1e-3, msg="sum d^2")
    assert torch.equal(ops.ssim(pg, td), got)                                   # fixed-order reductions: the same bits again


def test_repeated_calls_give_the_same_bits(ops):
    npz, pred, tgt = _inputs("odd")
    td = tgt.to(DEV)
    for lt in ("Fusion6", "L1_ssim_freq"):
        runs = [ops.loss_value_grad_stats(pred.to(DEV), td, lt) for _ in range(3)]
        for l, st, g in runs[1:]:
            assert l.item() == runs[0][0].item() and torch.equal(st, runs[0][1]) and torch.equal(g, runs[0][2])


@pytest.mark.parametrize("shape", [(1, 3, 40, 56), (2, 3, 180, 270)])
def test_identical_images(ops, shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    for lt in SSIM_TYPES:
        pg = x.clone().requires_grad_(True)
        loss, stats = ops.loss_with_stats(pg, x, lt)
        g, = torch.autograd.grad(loss, [pg])
        assert abs(loss.item()) < 1e-6, (lt, loss.item())
        assert torch.isfinite(g).all(), lt
        assert float((stats[:, 3] - 1).abs().max()) < 1e-6


def test_value_only_call_leaves_the_gradient_maps_alone(ops):
    """A value-only call (grad == NULL) must not write the statistic-gradient maps: the workspace region that holds them keeps a fill
    pattern through the call (C ABI, the library's own workspace layout: the maps follow the [B][512][2] sums)."""
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    npz, pred, tgt = _inputs("sub160")
    pg, td = pred.to(DEV), tgt.to(DEV)
    B, Cc, H, W = pg.shape
    lib = L.load()
    nbytes = lib.bnerv_loss_ssim_ws_bytes(B, Cc, H, W, 0)
    ws = torch.full((nbytes // 4,), -7.0, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, device=DEV); stats = torch.empty(B, L.LOSS_STATS, device=DEV)
    d = L.LossDesc(L.ptr(pg), L.ptr(td), None, L.ptr(loss), L.ptr(stats), L.ptr(ws), nbytes, B, Cc, H, W, 0.7, 0.0, 0.0, 0.0)
    L.check(lib.bnerv_loss_ssim_fwd_bwd(L.stream(), C.byref(d), 0.3), "bnerv_loss_ssim_fwd_bwd")
    ref, _ = ops.loss_with_stats(pg, td, "Fusion6")
    assert loss.item() == ref.item()
    maps = ws[B * 512 * 2: B * 512 * 2 + 3 * pg.numel()]
    assert bool((maps == -7.0).all())
    grad = torch.empty_like(pg)
    d.grad = L.ptr(grad).value
    L.check(lib.bnerv_loss_ssim_fwd_bwd(L.stream(), C.byref(d), 0.3), "bnerv_loss_ssim_fwd_bwd")
    assert not bool((maps == -7.0).all()) and torch.equal(grad, ops.loss_value_grad_stats(pg, td, "Fusion6")[2])
    d.c_ms = 0.3                                                                  # an MS-SSIM coefficient is refused
    assert lib.bnerv_loss_ssim_fwd_bwd(L.stream(), C.byref(d), 0.3) != 0


def test_fft_prepare_keeps_its_radix_limit():
    """bnerv_fft_prepare refuses a prime factor above BNERV_FFT_MAX_RADIX (31) as it always did; the wider limit (37, the 11 x 37 edge
    case) belongs to the SSIM path's own bnerv_loss_ssim_prepare."""
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    assert lib.bnerv_fft_prepare(11, 37) != 0 and lib.bnerv_fft_prepare(11, 31) == 0
    assert lib.bnerv_loss_ssim_prepare(11, 37) == 0 and lib.bnerv_loss_ssim_prepare(11, 41) != 0


@pytest.mark.parametrize("tag", ["720p", "1080p"])
def test_full_size_against_goldens(ops, tag):
    npz = load_golden("loss_ssim.npz")
    pred, tgt = _seeded(npz, tag)
    td = tgt.to(DEV)
    for lt in ("Fusion6", "L1_ssim_freq"):
        pg = pred.to(DEV).requires_grad_(True)
        loss, stats = ops.loss_with_stats(pg, td, lt)
        gold = float(npz[f"{tag}/{lt}/loss"])
        gg, = torch.autograd.grad(loss, [pg])
        idx, val = torch.from_numpy(npz[f"{tag}/{lt}/grad.idx"]), torch.from_numpy(npz[f"{tag}/{lt}/grad.val"])
        got = gg.flatten().cpu()[idx]
        print(f"{tag} {lt}: loss {loss.item():.8f} golden {gold:.8f}; max|grad sample err| {float((got - val).abs().max()):.3e} of {float(val.abs().max()):.3e}")
        assert abs(loss.item() - gold) <= 2e-4 * abs(gold), (lt, loss.item(), gold)
        close(got, val, rtol=2e-3, atol=2e-3 * float(val.abs().max()), msg=f"{tag} {lt} grad samples")
        close(stats[:, 3], torch.from_numpy(npz[f"{tag}/ssim_b"]), rtol=1e-4, atol=1e-5, msg=f"{tag} ssim_b")
        assert torch.equal(stats[:, 3], ops.ssim(pg, td))


# ----------------------------------------------------------------------------------------------------------- the train step
def _tiny_hnerv(sd=None):
    from boosting_nerv_amd.model_hnerv import HNeRV
    torch.manual_seed(1)
    model = HNeRV(hnerv_ref.tiny_args())
    if sd is not None:
        model.load_state_dict(sd)
    return model.to(DEV)


def _clip():
    from boosting_nerv_amd.synth import SyntheticVideo
    vid = SyntheticVideo(2, 180, 320)
    return torch.stack([vid.frame(i) for i in range(2)])


def _run_fusion6(use_graph, frames, order, sd0, steps):
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adam
    model = _tiny_hnerv(sd0)
    opt = Adam(model.parameters(), lr=1e-3)
    step = TrainStep(model, opt, "Fusion6", True, (1, 3, 180, 320), torch.device(DEV), use_graph=use_graph, warmup_eager=2)
    fd = frames.to(DEV)
    nd = torch.tensor([0.5, 1.0], dtype=torch.float64, device=DEV)
    losses, psnrs = [], []
    for s in range(steps):
        fi = order[s % len(order)]
        loss, psnr = step(fd[fi:fi + 1], nd[fi:fi + 1])
        losses.append(loss.item())
        psnrs.append(psnr.item())
    if use_graph:
        assert step.graph_a is not None
    return losses, psnrs, {k: v.detach().clone() for k, v in model.state_dict().items()}, model


def test_captured_fusion6_step_equals_eager_bit_for_bit():
    sd0 = group(load_golden("hnerv_base_tiny.npz"), "sd/")
    order = load_golden("hnerv_base_traj.npz")["order"].tolist()
    runs = {g: _run_fusion6(g, _clip(), order, sd0, 8) for g in (False, True)}
    assert runs[False][0] == runs[True][0] and runs[False][1] == runs[True][1]
    for k in runs[False][2]:
        assert torch.equal(runs[False][2][k], runs[True][2][k]), k
    assert runs[True][0][-1] < runs[True][0][0]                               # and it descends


def test_fusion6_short_schedule_end_psnr_matches_stock_ops():
    """40 Adam steps of the tiny HNeRV with Fusion6 over two frames: end PSNR of the HIP path against the same schedule restated with
    stock ops on the CPU (tests/hnerv_ref.py + msssim_ref.ssim), within the project's +-0.02 dB."""
    sd0 = group(load_golden("hnerv_base_tiny.npz"), "sd/")
    order = load_golden("hnerv_base_traj.npz")["order"].tolist()
    frames = _clip()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd0.items()}
    adam = hnerv_ref.AdamState(list(sd.values()), lr=1e-3)
    for s in range(40):
        fr = frames[order[s % len(order)]][None]
        img = hnerv_ref.forward(sd, fr)
        loss = (0.7 * F.l1_loss(img, fr, reduction="none").flatten(1).mean(1) + 0.3 * (1 - msssim_ref.ssim(img, fr, data_range=1, size_average=False))).mean()
        adam.step(torch.autograd.grad(loss, adam.params))
    with torch.no_grad():
        ref = float(np.mean([cpu_ref.psnr_fn_single(hnerv_ref.forward(sd, frames[i:i + 1]), frames[i:i + 1]).item() for i in range(2)]))
    _, _, _, model = _run_fusion6(True, frames, order, sd0, 40)
    from boosting_nerv_amd import hnerv_utils as hu
    with torch.no_grad():
        fd = frames.to(DEV)
        got = float(np.mean([hu.psnr_fn_single(model(fd[i:i + 1])[0], fd[i:i + 1]).item() for i in range(2)]))
    print(f"Fusion6 end PSNR after 40 steps: HIP {got:.4f} dB, stock ops {ref:.4f} dB")
    assert abs(got - ref) <= 0.02, (got, ref)


def test_boosted_model_takes_a_fusion6_step():
    from oracle import configs
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    from boosting_nerv_amd.optimizer import Adan
    frame = torch.rand(1, 3, 180, 320, generator=torch.Generator().manual_seed(5)).to(DEV)
    nd = torch.tensor([3 / 7], dtype=torch.float64, device=DEV)
    res = {}
    for use_graph in (False, True):
        torch.manual_seed(1)
        model = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
        step = TrainStep(model, Adan(model.parameters(), lr=0.003), "Fusion6", False, (1, 3, 180, 320), torch.device(DEV), use_graph=use_graph, warmup_eager=1)
        res[use_graph] = [tuple(v.item() for v in step(frame, nd)) for _ in range(4)]
    assert res[False] == res[True]
    assert res[True][-1][0] < res[True][0][0] and all(np.isfinite(v) for r in res[True] for v in r)


# --------------------------------------------------------------------------------------------------------------------- CLI
HNERV_FLAGS = ("--data_path synthetic:6x180x320 --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none "
               "--crop_list 180_320 --resize_list -1 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 "
               "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 --eval_freq 3 -p 2")


def _cli_default_loss(tmp_path, monkeypatch, extra):
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    seen = {}
    orig = T.TrainStep

    class Spy(orig):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["step"] = self
    monkeypatch.setattr(T, "TrainStep", Spy)
    assert "--loss" not in HNERV_FLAGS
    T.main((HNERV_FLAGS + " --outf t -e 3 --not_resume" + extra).split())
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    log = (out / "rank0.txt").read_text()
    assert "Eval at epoch 3" in log and "Training complete in" in log
    train_psnrs = [float(l.split("pred_PSNR: ")[1]) for l in log.splitlines() if "pred_PSNR" in l]
    print("train PSNR per logged line:", train_psnrs)
    assert train_psnrs[-1] > train_psnrs[0]
    return seen.get("step")


@pytest.mark.isolated
def test_hnerv_cli_trains_with_the_default_loss(tmp_path, monkeypatch):
    """The HNeRV recipe WITHOUT --loss (the CLI's default, Fusion6) on a synthetic clip, captured step."""
    step = _cli_default_loss(tmp_path, monkeypatch, "")
    assert step is not None and step.loss_type == "Fusion6" and step.graph_a is not None


@pytest.mark.isolated
def test_hnerv_cli_trains_with_the_default_loss_no_graph(tmp_path, monkeypatch):
    step = _cli_default_loss(tmp_path, monkeypatch, " --no_graph")
    assert step is None or step.graph_a is None


@pytest.mark.isolated
def test_compression_cli_with_fusion6(tmp_path, monkeypatch):
    """train_nerv_compression.py on a tiny synthetic clip with --loss Fusion6: the rate-distortion step takes the SSIM loss."""
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
             "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion6 --embed pe_1.25_80 "
             "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
             "-e 2 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
             "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1")
    C.main(flags.split())
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    psnrs = [float(x.split("pred_PSNR: ")[1].split()[0].rstrip(",")) for x in log.splitlines() if "pred_PSNR: " in x and "Epoch[" in x]
    assert "Eval at epoch 2" in log and len(psnrs) >= 2 and all(np.isfinite(psnrs)), log[-2000:]
