"""GPU parity tests (``-m gpu``) of the HNeRV baseline: the up-conv operator (5x5 family of csrc/conv5.hip, GELU around the 1x1 / 3x3
stages) against float64 stock ops, the f32 contract of the 5x5 kernels, the model against golden vectors of the REAL reference
(tools/make_hnerv_goldens.py), the fused Adam eager and captured, DecodeGraph, and the train script's CLI."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hnerv_ref
from conftest import ROOT, check_summary, group, load_golden
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Cin, Cout, H, W, k, s, act): the three H1 5x5 layers at reduced area with ragged edges, narrow layers, the 15M width, B = 2,
# stride 1 with and without GELU, and the H1 / UVG 1x1 and 3x3 stages with GELU
SHAPES = [
    (1, 67, 224, 19, 37, 5, 2, "gelu"), (1, 56, 188, 23, 70, 5, 2, "gelu"), (1, 47, 156, 45, 83, 5, 2, "gelu"),
    (1, 6, 6, 21, 45, 5, 1, "gelu"), (1, 7, 24, 13, 50, 5, 2, "gelu"), (1, 206, 688, 9, 20, 5, 2, "gelu"),
    (2, 33, 64, 17, 40, 5, 2, "gelu"), (2, 20, 20, 12, 33, 5, 1, "none"), (1, 39, 39, 30, 64, 5, 1, "gelu"), (1, 12, 48, 8, 32, 5, 2, "none"),
    (1, 96, 2000, 9, 16, 1, 5, "gelu"), (1, 86, 648, 15, 28, 3, 3, "gelu"), (1, 80, 268, 45, 80, 3, 2, "gelu"), (1, 16, 96, 9, 16, 1, 1, "gelu"),
]


def _ref_upconv(x, w, b, s, act):
    y = F.conv2d(x, w, b, padding=(w.shape[-1] - 1) // 2)
    y = F.pixel_shuffle(y, s) if s > 1 else y
    return F.gelu(y) if act == "gelu" else y


def _operator_case(B, Cin, Cout, H, W, k, s, act, seed=0):
    from boosting_nerv_amd import ops
    g = torch.Generator().manual_seed(1000 * Cin + Cout + seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g) * 0.2
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    out = ops.upconv_act(*leaves, s, act)
    cot = torch.randn(out.shape, generator=g)
    grads = torch.autograd.grad(out, leaves, cot.to(DEV))
    ld = [t.double().requires_grad_(True) for t in (x, w, b)]
    ref = _ref_upconv(*ld, s, act)
    rgrads = torch.autograd.grad(ref, ld, cot.double())
    tag = f"{Cin}->{Cout} k{k} s{s} {act} @{H}x{W} B{B}"
    close(out, ref, msg=f"fwd {tag}")
    for n, a, r in zip(("dx", "dw", "db"), grads, rgrads):
        close(a, r, msg=f"{n} {tag}")
    with torch.no_grad():                                   # decode form (nothing saved): the same bits
        assert torch.equal(ops.upconv_act(leaves[0], leaves[1], leaves[2], s, act), out)
    # first layer of a model: no input gradient requested
    o2 = ops.upconv_act(leaves[0].detach(), leaves[1], leaves[2], s, act)
    dw2, db2 = torch.autograd.grad(o2, leaves[1:], cot.to(DEV))
    assert torch.equal(dw2, grads[1]) and torch.equal(db2, grads[2])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_upconv_act_matches_float64_stock_ops(shape):
    _operator_case(*shape)


def test_upconv_act_full_size_h1_last_stage():
    _operator_case(1, 47, 156, 360, 640, 5, 2, "gelu")


def test_conv2d_ps_routes_5x5_and_module_runs():
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.model_blocks import UpConv
    torch.manual_seed(2)
    up = UpConv(ngf=9, new_ngf=5, strd=2, ks=5, conv_type="pshuffel", bias=True, args=hnerv_ref.tiny_args()).to(DEV)
    x = torch.randn(1, 9, 11, 19, device=DEV)
    c = up.conv_module()
    ref = F.pixel_shuffle(F.conv2d(x.double().cpu(), c.weight.double().cpu(), c.bias.double().cpu(), padding=2), 2)
    close(up(x), ref, msg="fwd UpConv k5")
    close(ops.conv2d_ps(x, c.weight, c.bias, 2), ref, msg="fwd conv2d_ps k5")


def test_5x5_kernels_keep_the_f32_contract():
    """tools/split_contract.py --only k5: |kernel - float64| <= 3.5e-7 * sum|a||b| per element for the forward, data, weight and bias
    gradient launches of the 5x5 family in the default bf16x6 arithmetic; the same check must fail under BNERV_SPLIT_WIDE=bf16x3."""
    tool = os.path.join(ROOT, "tools", "split_contract.py")
    env = dict(os.environ)
    env.pop("BNERV_SPLIT_WIDE", None)
    r6 = subprocess.run([sys.executable, tool, "--only", "k5"], capture_output=True, text=True, timeout=600, env=env)
    print(r6.stdout[-3000:])
    assert r6.returncode == 0 and "k5" in r6.stdout, r6.stdout[-3000:] + r6.stderr[-2000:]
    env["BNERV_SPLIT_WIDE"] = "bf16x3"
    r3 = subprocess.run([sys.executable, tool, "--only", "k5"], capture_output=True, text=True, timeout=600, env=env)
    print(r3.stdout[-3000:])
    assert r3.returncode == 1 and "OUTSIDE" in r3.stdout, r3.stdout[-3000:] + r3.stderr[-2000:]


def _tiny_model(sd=None):
    from boosting_nerv_amd.model_hnerv import HNeRV
    torch.manual_seed(1)
    model = HNeRV(hnerv_ref.tiny_args())
    if sd is not None:
        model.load_state_dict(sd)
    return model.to(DEV)


def test_tiny_model_against_reference_golden():
    from boosting_nerv_amd import hnerv_utils as hu
    npz = load_golden("hnerv_base_tiny.npz")
    sd = group(npz, "sd/")
    model = _tiny_model()
    for k, v in model.state_dict().items():                 # init ORDER parity (decoder bit for bit; the encoder's trunc_normal_ depends on the host ISA)
        if k.startswith("encoder."):
            torch.testing.assert_close(v.cpu(), sd[k], rtol=0, atol=1e-6, msg=k)
        else:
            assert torch.equal(v.cpu(), sd[k]), k
    model.load_state_dict(sd)
    frame = torch.rand(1, 3, 180, 320, generator=torch.Generator().manual_seed(int(npz["frame_seed"]))).to(DEV)
    img, lst, _ = model(frame)
    check_summary(img, npz, "img", 1e-3, 1e-5)
    assert len(lst) == 6
    for i, t in enumerate(lst):
        check_summary(t, npz, f"list{i}", 1e-3, 2e-5)
    loss = hu.loss_fn(img, frame, "L2")
    gold = float(npz["loss_L2"])
    assert abs(loss.item() - gold) < 3e-4 * abs(gold), (loss.item(), gold)
    torch.testing.assert_close(hu.psnr_fn_single(img, frame).cpu(), torch.from_numpy(npz["psnr"]), rtol=1e-4, atol=2e-3)
    loss.backward()
    for k, p in model.named_parameters():
        gn = float(npz[f"gnorm/{k}"])
        got = p.grad.double().norm().item()
        assert abs(got - gn) <= 5e-3 * gn + 1e-6, (k, got, gn)
        ref = torch.from_numpy(npz[f"grad/{k}"])
        err = (p.grad.cpu() - ref).abs().max().item()
        assert err <= 5e-3 * max(gn, float(ref.abs().max())) + 1e-6, (k, err, gn)


def test_h1_full_size_against_reference_golden():
    """regression/bunny/hnerv.sh at 1.525 M (fc_dim 96), 720x1280: the decoder from a stored 16x9x16 embedding (the encoder is exempt from
    bit tests across CPU ISAs), seeded parameters identical to the reference's (SHA-256), activations, loss, PSNR, decoder gradients."""
    from boosting_nerv_amd import hnerv_utils as hu
    from boosting_nerv_amd.model_hnerv import HNeRV
    npz = load_golden("hnerv_base_h1.npz")
    torch.manual_seed(1)
    model = HNeRV(hnerv_ref.h1_args())
    assert hnerv_ref.decoder_sha(model.state_dict()) == str(npz["decoder_sha256"])
    model = model.to(DEV)
    embed = torch.from_numpy(npz["embed"]).to(DEV).requires_grad_(True)
    frame = torch.rand(1, 3, 720, 1280, generator=torch.Generator().manual_seed(int(npz["frame_seed"]))).to(DEV)
    img, lst, _ = model(frame, input_embed=embed)
    check_summary(img, npz, "img", 1e-3, 1e-5)
    for i, t in enumerate(lst):
        check_summary(t, npz, f"list{i}", 1e-3, 2e-5)
    loss = hu.loss_fn(img, frame, "L2")
    gold = float(npz["loss_L2"])
    assert abs(loss.item() - gold) < 3e-4 * abs(gold), (loss.item(), gold)
    torch.testing.assert_close(hu.psnr_fn_single(img, frame).cpu(), torch.from_numpy(npz["psnr"]), rtol=1e-4, atol=2e-3)
    loss.backward()
    for k, p in model.named_parameters():
        if k.startswith("encoder."):
            assert p.grad is None
            continue
        gn = float(npz[f"gnorm/{k}"])
        got = p.grad.double().norm().item()
        assert abs(got - gn) <= 5e-3 * gn + 1e-9, (k, got, gn)
        check_summary(p.grad, npz, f"grad/{k}", rtol=2e-3, atol=1e-4 * gn + 1e-9)


def _run_traj(use_graph, frames, order, sd0, steps=None):
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adam
    model = _tiny_model(sd0)
    opt = Adam(model.parameters(), lr=1e-3)
    step = TrainStep(model, opt, "L2", True, (1, 3, 180, 320), torch.device(DEV), use_graph=use_graph, warmup_eager=2)
    fd = frames.to(DEV)
    nd = torch.tensor([0.5, 1.0], dtype=torch.float64, device=DEV)
    losses, psnrs = [], []
    for s in range(steps or len(order)):
        fi = order[s % len(order)]
        loss, psnr = step(fd[fi:fi + 1], nd[fi:fi + 1])
        losses.append(loss.item())
        psnrs.append(psnr.item())
    if use_graph:
        assert step.graph_a is not None
    return losses, psnrs, {k: v.detach().clone() for k, v in model.state_dict().items()}, model


def _clip():
    from boosting_nerv_amd.synth import SyntheticVideo
    vid = SyntheticVideo(2, 180, 320)
    return torch.stack([vid.frame(i) for i in range(2)])


def test_fused_adam_trajectory_matches_reference_eager_and_captured():
    """8 torch.optim.Adam(lr=1e-3) steps of the REAL reference (tiny model, 2 synthetic frames): loss 2e-3 relative and PSNR 0.02 dB per
    step, final parameters max <= 0.1 sum(lr), mean <= 2e-5 per tensor; the captured step equals the eager one bit for bit."""
    npz = load_golden("hnerv_base_traj.npz")
    sd0 = group(load_golden("hnerv_base_tiny.npz"), "sd/")
    order = npz["order"].tolist()
    runs = {}
    for use_graph in (False, True):
        losses, psnrs, final, _ = _run_traj(use_graph, _clip(), order, sd0)
        runs[use_graph] = (losses, psnrs, final)
        for s in range(len(order)):
            print(f"graph={use_graph} step {s}: loss {losses[s]:.8f} (ref {npz['loss'][s]:.8f}) psnr {psnrs[s]:.5f} (ref {npz['psnr'][s]:.5f})")
        for s in range(len(order)):
            assert abs(losses[s] - npz["loss"][s]) <= 2e-3 * abs(npz["loss"][s]), (use_graph, s, losses[s], npz["loss"][s])
            assert abs(psnrs[s] - npz["psnr"][s]) <= 0.02, (use_graph, s, psnrs[s], npz["psnr"][s])
        for k, v in final.items():
            d = (v.cpu() - torch.from_numpy(npz[f"final/{k}"])).abs()
            assert d.max().item() <= 0.1 * 8 * 1e-3, (k, d.max().item())
            assert d.mean().item() <= 2e-5, (k, d.mean().item())
    assert runs[False][0] == runs[True][0] and runs[False][1] == runs[True][1]
    for k in runs[False][2]:
        assert torch.equal(runs[False][2][k], runs[True][2][k]), k


def test_fused_adam_equals_stock_adam_on_the_same_gradients():
    from boosting_nerv_amd.optimizer import Adam
    g = torch.Generator().manual_seed(4)
    shapes = [(156, 47, 5, 5), (156,), (3, 39, 3, 3), (1,), (2000, 96, 1, 1)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours, stock = Adam(ps, lr=2e-3), torch.optim.Adam(qs, lr=2e-3, foreach=False)
    for it in range(5):
        for p, q in zip(ps, qs):
            p.grad = (torch.randn(p.shape, generator=g) * 10.0 ** (it - 3)).to(DEV)
            q.grad = p.grad.clone()
        ours.step(); stock.step()
    for p, q in zip(ps, qs):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7)
    sd = ours.state_dict()
    assert float(sd["state"][0]["step"]) == 5.0
    torch.testing.assert_close(sd["state"][0]["exp_avg_sq"], stock.state_dict()["state"][0]["exp_avg_sq"], rtol=1e-6, atol=1e-12)


def test_decode_graph_equals_eager_decode_and_follows_the_weights():
    from boosting_nerv_amd.engine import DecodeGraph
    model = _tiny_model().eval()
    frames = torch.rand(3, 1, 3, 180, 320, generator=torch.Generator().manual_seed(9)).to(DEV)
    norm = torch.tensor([0.5], dtype=torch.float64, device=DEV)
    with torch.no_grad():
        embeds = [model(frames[i])[1][0] for i in range(3)]
        dg = DecodeGraph(model, frames[0], embeds[0], norm)
        for i in (1, 2, 0):
            ref = model(frames[i], embeds[i], norm_idx=norm)[0]
            out, dt = dg(frames[i], embeds[i], norm)
            assert dt > 0 and torch.equal(out, ref), (i, float((out - ref).abs().max()))
        for p in model.parameters():
            p.mul_(1.03)
        ref = model(frames[1], embeds[1], norm_idx=norm)[0]
        dg.refresh()
        out = dg(frames[1], embeds[1], norm)[0]
        assert torch.equal(out, ref), float((out - ref).abs().max())


def test_short_schedule_end_psnr_matches_stock_ops():
    """40 Adam steps over the two frames: end PSNR of the HIP path against tests/hnerv_ref.py on the CPU (and the reference's own figure
    in the golden), within the project's +-0.02 dB."""
    npz = load_golden("hnerv_base_traj.npz")
    sd0 = group(load_golden("hnerv_base_tiny.npz"), "sd/")
    frames = _clip()
    order = npz["order"].tolist()
    _, _, final_ref = hnerv_ref.trajectory(sd0, frames, [order[s % len(order)] for s in range(40)])
    from oracle import cpu_ref
    with torch.no_grad():
        ref = float(np.mean([cpu_ref.psnr_fn_single(hnerv_ref.forward(final_ref, frames[i:i + 1]), frames[i:i + 1]).item() for i in range(2)]))
    _, _, _, model = _run_traj(True, frames, order, sd0, steps=40)
    from boosting_nerv_amd import hnerv_utils as hu
    with torch.no_grad():
        fd = frames.to(DEV)
        got = float(np.mean([hu.psnr_fn_single(model(fd[i:i + 1])[0], fd[i:i + 1]).item() for i in range(2)]))
    print(f"end PSNR after 40 steps: HIP {got:.4f} dB, stock ops {ref:.4f} dB, reference {float(npz['end_psnr_40']):.4f} dB")
    assert abs(ref - float(npz["end_psnr_40"])) <= 0.02
    assert abs(got - ref) <= 0.02, (got, ref)


@pytest.mark.isolated
def test_baseline_cli_end_to_end(tmp_path, monkeypatch):
    """train_nerv_all.py with the regression recipe's flags at tiny strides on a synthetic clip: 3 epochs on the captured step with the
    fused Adam, the artefacts, resume, --eval_only reproducing the logged metrics; one epoch each of the interpolation and inpainting forms."""
    import csv
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    base = ("--data_path synthetic:6x180x320 --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none "
            "--crop_list 180_320 --resize_list -1 --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 "
            "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 --eval_freq 3 -p 2")
    seen = {}
    orig = T.TrainStep

    class Spy(orig):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["step"] = self
    monkeypatch.setattr(T, "TrainStep", Spy)
    T.main((base + " --outf t -e 3 --not_resume").split())
    assert type(seen["step"].opt).__name__ == "Adam" and seen["step"].graph_a is not None      # the captured step with the fused Adam
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    for f in ("args.yaml", "rank0.txt", "model_latest.pth", "epoch3.csv"):
        assert (out / f).is_file(), f
    log = (out / "rank0.txt").read_text()
    assert "Eval at epoch 3" in log and "bits per pixel" in log and "Training complete in" in log
    rows = list(csv.reader(open(out / "epoch3.csv")))
    rec = dict(zip(rows[0][1:], rows[1][1:]))
    psnr, qpsnr = float(rec["pred_seen_psnr"]), float(rec["quant_seen_psnr"])
    assert 8.0 < psnr < 60.0 and abs(psnr - qpsnr) < 1.0 and float(rec["bits/pixel"]) > 0
    train_psnrs = [float(l.split("pred_PSNR: ")[1]) for l in log.splitlines() if "pred_PSNR" in l]
    assert train_psnrs[-1] > train_psnrs[0]
    ck = torch.load(out / "model_latest.pth", map_location="cpu")
    assert set(ck["optimizer"]["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}                 # torch.optim.Adam's layout
    T.main((base + " --outf t -e 3 --eval_only").split())
    rows = list(csv.reader(open(out / "eval.csv")))
    rec2 = dict(zip(rows[0][1:], rows[1][1:]))
    assert abs(float(rec2["pred_seen_psnr"]) - psnr) < 0.02 and abs(float(rec2["quant_seen_psnr"]) - qpsnr) < 0.05
    T.main((base + " --outf t -e 4").split())                                                     # resumes from epoch 3
    assert "Epoch[4/4]" in (out / "rank0.txt").read_text()
    T.main((base + " --outf ti -e 1 --not_resume --interpolation --data_split 1_1_2 --embed_inter").split())
    assert "Eval at epoch 1" in (tmp_path / "output" / "ti" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    T.main((base + " --outf tp -e 1 --not_resume --inpanting inpanting_center --clip_max_norm 1").split())
    assert "Eval at epoch 1" in (tmp_path / "output" / "tp" / "tiny" / "Size0.05" / "rank0.txt").read_text()
