"""Inpainting on the HIP path: the mask kernels (bnerv_inpaint_head / _pred / _psnr / _grad) behind the mask= argument of the loss entry
points, the masked train step (eager and captured) against the reference's own masked step (tests/golden/inpaint.npz), and the two
inpainting recipe lines of the CLI on the captured step.

The masked loss is loss(pred * mask, gt * mask) of the unchanged loss kernels on products that are single fp32 multiplies, so value and
gradient are compared with torch.equal; the PSNR against the unmasked frame and the golden comparisons use the tolerances of the existing
eager test (tests/test_gpu_models.py test_inpainting_masked_step_against_reference_golden)."""
import argparse
import copy

import numpy as np
import pytest
import torch

from conftest import group, load_golden
from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = ("inpanting_center", "inpanting_fixed_50")


def _mask(mode, H, W):
    from boosting_nerv_amd import hnerv_utils as hu
    m = hu.TransformInput(argparse.Namespace(inpanting=mode))(torch.zeros(1, 3, H, W, device=DEV), None)[2]
    assert m.shape == (H, W) and 0 < int((m == 0).sum()) < H * W
    return m


def _shifted(t, k=1):
    """Same values, contiguous, k elements past a 16-byte boundary (tests/test_gpu_alignment.py `shifted`)."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf.fill_(NAN)
    v = buf[k:k + n].view(t.shape)
    v.copy_(t.detach())
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
    return v.detach().requires_grad_(t.requires_grad), buf


def _masked_pair(ops, pred, gt, m, lt):
    """-> (loss, stats, pred.grad) of the mask= form and of the same loss on explicit products."""
    a = pred.detach().clone().requires_grad_(True)
    la, sa = ops.loss_with_stats(a, gt, lt, mask=m)
    la.backward()
    b = pred.detach().clone().requires_grad_(True)
    lb, sb = ops.loss_with_stats(b * m, gt * m, lt)
    lb.backward()
    return (la.detach(), sa, a.grad), (lb.detach(), sb, b.grad)


def _check(ops, pred, gt, m, lt):
    (la, sa, ga), (lb, sb, gb) = _masked_pair(ops, pred, gt, m, lt)
    assert torch.equal(la, lb), (lt, la.item(), lb.item())
    assert torch.equal(ga, gb), lt
    assert torch.equal(sa[:, :4], sb[:, :4])                                   # the loss's own columns are those of the masked pair ...
    want = ops.psnr(pred, gt)                                                  # ... and column 4 is the PSNR against the UNMASKED frame
    print(f"{lt} {tuple(pred.shape)}: psnr {sa[:, 4].tolist()} unmasked reference {want.tolist()} (masked pair {sb[:, 4].tolist()})")
    torch.testing.assert_close(sa[:, 4], want, rtol=1e-4, atol=2e-3)
    assert not torch.allclose(sb[:, 4], want, rtol=1e-4, atol=2e-3)            # (the masked pair's PSNR is another number)
    # the step's entry point: same loss, the gradient already masked, target_masked handed in
    gt_m, _ = ops.inpaint_head(gt, m)
    l2, s2, g2 = ops.loss_value_grad_stats(pred, gt, lt, mask=m, target_masked=gt_m)
    assert torch.equal(l2, la) and torch.equal(g2, ga) and torch.equal(s2, sa)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lt", ["L2", "Fusion6", "Fusion10_freq"])
def test_masked_loss_equals_the_loss_of_the_products(lt, mode):
    from boosting_nerv_amd import ops
    g = torch.Generator().manual_seed(3)
    pred = torch.rand(2, 3, 180, 320, generator=g).to(DEV)
    gt = torch.rand(2, 3, 180, 320, generator=g).to(DEV)
    _check(ops, pred, gt, _mask(mode, 180, 320), lt)


@pytest.mark.parametrize("mode", MODES)
def test_masked_loss_on_a_frame_size_that_is_no_multiple_of_four(mode):
    from boosting_nerv_amd import ops
    g = torch.Generator().manual_seed(4)
    pred, gt = torch.rand(2, 3, 13, 17, generator=g).to(DEV), torch.rand(2, 3, 13, 17, generator=g).to(DEV)
    m = torch.ones(13, 17, device=DEV)
    if "center" in mode:
        m[5:8, 6:10] = 0
    else:
        m[2:4, 3:5] = 0; m[9:11, 12:14] = 0
    _check(ops, pred, gt, m, "L2")


@pytest.mark.parametrize("mode", MODES)
def test_masked_loss_on_operands_four_bytes_off_a_16_byte_boundary(mode):
    from boosting_nerv_amd import ops
    g = torch.Generator().manual_seed(5)
    pred, gt = torch.rand(2, 3, 180, 320, generator=g).to(DEV), torch.rand(2, 3, 180, 320, generator=g).to(DEV)
    m = _mask(mode, 180, 320)
    (l0, s0, g0), _ = _masked_pair(ops, pred, gt, m, "L2")
    ps, pb = _shifted(pred.requires_grad_(True))
    gs, gb = _shifted(gt)
    ms, mb = _shifted(m)
    l1, s1 = ops.loss_with_stats(ps, gs, "L2", mask=ms)
    l1.backward()
    assert torch.equal(l1.detach(), l0) and torch.equal(ps.grad, g0) and torch.equal(s1, s0)      # the scalar form gives the same bits
    for buf, n in ((pb, pred.numel()), (gb, gt.numel()), (mb, m.numel())):
        b = buf.cpu()
        assert torch.isnan(b[:1]).all() and torch.isnan(b[1 + n:]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,k", [((2, 3, 180, 320), 0), ((2, 3, 13, 17), 0), ((1, 3, 180, 320), 1)])
def test_head_kernel_is_exactly_transform_input(shape, k, mode):
    from boosting_nerv_amd import ops
    frame = (torch.rand(shape, generator=torch.Generator().manual_seed(5)) * 1.2 - 0.1).to(DEV)
    assert frame.min() < 0 and frame.max() > 1
    m = _mask(mode, 180, 320) if shape[-1] == 320 else (torch.rand(13, 17, device=DEV) > 0.3).float()
    if k:
        frame, _ = _shifted(frame, k)
    gt_m, inp = ops.inpaint_head(frame, m, want_inp=True)
    assert torch.equal(gt_m, frame * m) and torch.equal(inp, (frame * m).clamp(min=0, max=1))
    gt_m2, none = ops.inpaint_head(frame, m)
    assert none is None and torch.equal(gt_m2, gt_m)


# ---- the masked step against the reference's -------------------------------------------------------------------------------------------
def _build(args):
    from boosting_nerv_amd.model_hnerv import HNeRV_Boost
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    return NeRV_Boost(1, args=args) if args.model == "NeRV_Boost" else HNeRV_Boost(args)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mname,cfg", [("nerv", configs.tiny_nerv), ("hnerv", configs.tiny_hnerv)])
def test_masked_train_step_against_reference_golden(mname, cfg, mode):
    """TrainStep(mask=...) with Adan at lr = 0 (parameters fixed, .grad survives the step), called four times: one eager call, the
    capture, two replays.  Loss, PSNR against the unmasked frame and every gradient norm against the reference's masked step
    (train_nerv_all.py:334-346), on the eager call and on a replayed one; eager and replayed loss bit-equal."""
    from boosting_nerv_amd import hnerv_utils as hu
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adan
    npz = load_golden("inpaint.npz")
    args = copy.copy(cfg())
    args.inpanting = mode
    torch.manual_seed(1)
    model = _build(args)
    model.load_state_dict({k: v for k, v in group(load_golden(f"tiny_{mname}.npz"), "sd/").items()})
    model = model.to(DEV)
    frame = (torch.rand(2, 3, 180, 320, generator=torch.Generator().manual_seed(5)) * 1.2 - 0.1).to(DEV)
    norm_idx = torch.tensor([3 / 7, 6 / 7], dtype=torch.float64, device=DEV)
    mask = hu.TransformInput(args)(frame, None)[2]
    k = f"{mname}/{mode}"
    assert np.array_equal(mask.cpu().numpy().astype(np.uint8), np.unpackbits(npz[f"{k}/mask"])[:180 * 320].reshape(180, 320))
    opt = Adan(model.parameters(), lr=0.0)
    step = TrainStep(model, opt, "L1_freq", args.model == "HNeRV_Boost", (2, 3, 180, 320), torch.device(DEV), use_graph=True, warmup_eager=1, mask=mask)
    gold = float(npz[f"{k}/loss_L1_freq"])
    losses = []
    for call in range(4):
        loss, psnr = step(frame, norm_idx)
        assert (step.graph_a is not None) == (call >= 1)
        losses.append(loss.clone())
        if call in (0, 3):                                                     # the eager call and a replayed one
            print(f"{k} call {call}: loss {loss.item()!r} (golden {gold!r}), psnr {psnr.tolist()} (golden {npz[f'{k}/psnr'].tolist()})")
            assert abs(loss.item() - gold) < 3e-4 * abs(gold), (call, loss.item(), gold)
            torch.testing.assert_close(psnr.cpu(), torch.from_numpy(npz[f"{k}/psnr"]), rtol=1e-4, atol=2e-3)
            for pn, p in model.named_parameters():
                gn = float(npz[f"{k}/gnorm/{pn}"])
                if gn < 0:
                    continue
                got = p.grad.double().norm().item()
                assert abs(got - gn) <= 5e-3 * gn + 1e-6, (call, pn, got, gn)
    assert torch.equal(losses[0], losses[3]) and torch.equal(losses[0], losses[2])
    if args.model == "HNeRV_Boost":                                            # the model read the masked, clamped frame
        assert torch.equal(step.static_in, (frame * mask).clamp(min=0, max=1))


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
NERV_LINE = ("--data_path synthetic:6x180x320 --vid tiny --model NeRV_Boost --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 "
             "--act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 "
             "--ks 0_3_3 --reduce 2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 --lr 0.003 --eval_freq 3 -p 2 --data_split 4_5_6 "
             "--optim_type Adan")
HNERV_LINE = ("--data_path synthetic:6x180x320 --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none "
              "--crop_list 180_320 --resize_list -1 --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 "
              "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 --eval_freq 3 -p 2")


@pytest.mark.isolated
@pytest.mark.parametrize("name,line,opt_name", [("nerv_boost", NERV_LINE, "Adan"), ("hnerv", HNERV_LINE, "Adam")])
def test_inpainting_recipes_run_on_the_captured_step(tmp_path, monkeypatch, name, line, opt_name):
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    seen = {}
    orig = T.TrainStep

    class Spy(orig):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["step"] = self
    monkeypatch.setattr(T, "TrainStep", Spy)
    T.main((line + " --outf ti -e 3 --not_resume --inpanting inpanting_fixed_50 --clip_max_norm 1").split())
    step = seen["step"]
    assert type(step.opt).__name__ == opt_name and step.mask is not None and step.clip_max_norm == 1 and step.graph_a is not None
    assert step.opt.clip_out is not None and 0 < step.opt.clip_out[1].item() <= 1
    out = tmp_path / "output" / "ti" / "tiny" / "Size0.05"
    log = (out / "rank0.txt").read_text()
    assert "Train step: captured" in log and "inpanting_fixed_50" in log
    assert "Epoch[3/3]" in log and "Eval at epoch 3" in log
    train_psnrs = [float(l.split("pred_PSNR: ")[1]) for l in log.splitlines() if "pred_PSNR" in l]
    assert train_psnrs[-1] > train_psnrs[0], train_psnrs
    ck = torch.load(out / "model_latest.pth", map_location="cpu")
    assert ck["epoch"] == 3 and ck["state_dict"] and ck["optimizer"]["state"]
