"""GPU tests (``-m gpu``) of the time-embedding branch's two-launch backward (include/bnerv.h bnerv_time_branch_bwd, csrc/dense.hip;
ops._TimeBranch.backward): bit-equal to the five grouped launches it replaces (BNERV_TIME_BRANCH_BWD=0), and -- so that the code is not
only compared with itself -- within the gradient bound of tests/test_gpu_ops.py, 1e-5 + 1e-4 max|ref|, of float64 autograd over stock ops.
Shapes sit on the kernels' edges, not at the model's size: one / two / three dx chunks of the stem (the last with 2 rows, a row count that
is no multiple of 4), modulation widths on both sides of the 64-row chunk and at the maximum, the largest group count, B up to the limit."""
import math
import types

import pytest
import torch

from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LV = 4      # I = 8


def _params(seed, SH, SO, TH, TO, widths):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh, sc=1.0: torch.randn(*sh, generator=g) * sc
    I = 2 * LV
    stem = [rn(SH, I, 1, 1, sc=0.4), rn(SH, sc=0.1), rn(SO, SH, 1, 1, sc=0.5 / math.sqrt(SH)), rn(SO, sc=0.1)]
    stem_t = [rn(TH, I, 1, 1, sc=0.4), rn(TH, sc=0.1), rn(TO, TH, 1, 1, sc=0.7 / math.sqrt(TH)), rn(TO, sc=0.1)]
    mlps = [[rn(TO, TO, 1, 1, sc=1.0 / math.sqrt(TO)), rn(TO, sc=0.3), rn(c, TO, 1, 1, sc=1.0 / math.sqrt(TO)), rn(c, sc=0.1)] for c in widths]
    return stem + stem_t + [t for m in mlps for t in m], g


def _bases_pos(B):
    bases = (1.25 ** torch.arange(LV, dtype=torch.float32)) * math.pi      # (moderate arguments: the PE itself is pinned elsewhere)
    pos = torch.tensor([(i + 1) / (B + 1) for i in range(B)], dtype=torch.float64)
    return bases, pos


def _reference(flat, bases, pos, n_mlp, cots, use_zt, unused):
    """float64 autograd over stock ops; a parameter no cotangent reaches has the gradient zero."""
    ps = [t.double().requires_grad_(True) for t in flat]
    arg = pos.float()[:, None] * bases[None, :]                            # the reference's single fp32 product (model_blocks.py:122)
    pe = torch.cat([torch.sin(arg), torch.cos(arg)], 1).double()
    lin = lambda x, w, b: x @ w.flatten(1).T + b
    so = torch.sin(lin(torch.sin(lin(pe, ps[0], ps[1])), ps[2], ps[3]))
    zt = torch.sin(lin(torch.sin(lin(pe, ps[4], ps[5])), ps[6], ps[7]))
    outs = [lin(torch.relu(lin(zt, ps[8 + 4 * i], ps[9 + 4 * i])), ps[10 + 4 * i], ps[11 + 4 * i]) for i in range(n_mlp)]
    heads, cs = [so], [cots[0].double()]
    if use_zt:
        heads.append(zt); cs.append(cots[1].double())
    for i in range(n_mlp):
        if i not in unused:
            heads.append(outs[i]); cs.append(cots[2 + i].double())
    gr = torch.autograd.grad(heads, ps, cs, allow_unused=True)
    return [torch.zeros_like(p) if g is None else g for g, p in zip(gr, ps)]


def _within_bound(got, ref, what):
    for i, (a, r) in enumerate(zip(got, ref)):
        a, r = a.detach().double().cpu().reshape(r.shape), r.detach()
        assert torch.isfinite(a).all(), f"{what}: gradient {i} is not finite"
        bound = 1e-5 + 1e-4 * float(r.abs().max())
        err = float((a - r).abs().max())
        assert err <= bound, f"{what}: gradient {i}: max abs err {err:.3e} > {bound:.3e} (ref max {float(r.abs().max()):.3e})"


# (SH, SO, TH, TO, B, widths, d_ty1 given, modulation outputs outside the loss)
W5 = [12, 59, 64, 65, 128]
CASES = [
    pytest.param(8, 6, 4, 4, 1, [4], False, (), id="smallest"),
    pytest.param(70, 130, 64, 32, 4, W5, True, (), id="extremes-wide"),
    pytest.param(70, 130, 64, 32, 4, [7] * 39, False, (), id="extremes-39-groups"),
    pytest.param(8, 70, 4, 32, 3, W5, False, (1, 3), id="two-outputs-unused"),
    pytest.param(70, 6, 64, 4, 1, [7] * 39, True, (), id="39-groups-narrow"),
    pytest.param(70, 70, 4, 4, 3, [4], True, (), id="two-chunks"),
]


@pytest.mark.parametrize("SH,SO,TH,TO,B,widths,use_zt,unused", CASES)
def test_two_launch_backward_has_the_bits_of_the_five_launch_form(SH, SO, TH, TO, B, widths, use_zt, unused, monkeypatch):
    from boosting_nerv_amd import ops
    n = len(widths)
    flat, g = _params(20 + SH + SO + n, SH, SO, TH, TO, widths)
    bases, pos = _bases_pos(B)
    cots = [torch.randn(B, SO, generator=g), torch.randn(B, TO, generator=g)] + [torch.randn(B, c, generator=g) for c in widths]
    ref = _reference(flat, bases, pos, n, cots, use_zt, unused)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BNERV_TIME_BRANCH_BWD", flag)
        pg = [t.to(DEV).requires_grad_(True) for t in flat]
        out = ops.time_branch(pos.to(DEV), bases.to(DEV), tuple(pg[:4]), tuple(pg[4:8]), [tuple(pg[8 + 4 * i:12 + 4 * i]) for i in range(n)])
        assert out is not None, "these shapes are the forward kernel's"
        heads, cs = [out[0]], [cots[0]]
        if use_zt:
            heads.append(out[1]); cs.append(cots[1])
        for i in range(n):
            if i not in unused:
                heads.append(out[2][i]); cs.append(cots[2 + i])
        before = dict(ops.TIME_BRANCH_BWD_CALLS)
        res[flag] = torch.autograd.grad(heads, pg, [c.to(DEV) for c in cs])
        after = ops.TIME_BRANCH_BWD_CALLS
        if flag == "1":         # (c) the entry point took these shapes
            assert (after["taken"], after["declined"]) == (before["taken"] + 1, before["declined"]), (before, after)
        else:
            assert after == before, "BNERV_TIME_BRANCH_BWD=0 must not reach the entry point"
    for i, (a, b) in enumerate(zip(res["1"], res["0"])):                   # (a) bit for bit
        assert a.shape == b.shape and torch.equal(a, b), f"gradient {i}: {int((a != b).sum())}/{a.numel()} differ, max {float((a - b).abs().max()):.3e}"
    _within_bound(res["1"], ref, "two launches")                           # (b) against float64
    _within_bound(res["0"], ref, "five launches")


@pytest.mark.parametrize("B,widths", [(5, [12, 7]), (2, [12, 129])])
def test_shapes_outside_the_limits_fall_back_to_the_five_launch_form(B, widths, monkeypatch):
    """The forward's gate (ops.time_branch) has the same limits, so such a branch reaches _TimeBranch.backward only with tensors saved by
    somebody else: here by stock fp32 torch ops.  The entry point must answer "not mine" and the five grouped launches must deliver."""
    from boosting_nerv_amd import ops
    monkeypatch.setenv("BNERV_TIME_BRANCH_BWD", "1")
    SH, SO, TH, TO, n = 70, 130, 64, 32, len(widths)
    flat, g = _params(77 + B, SH, SO, TH, TO, widths)
    bases, pos = _bases_pos(B)
    cots = [torch.randn(B, SO, generator=g), torch.randn(B, TO, generator=g)] + [torch.randn(B, c, generator=g) for c in widths]
    ref = _reference(flat, bases, pos, n, cots, True, ())
    p = [t.to(DEV).flatten(1) if t.dim() > 1 else t.to(DEV) for t in flat]
    arg = pos.float()[:, None].to(DEV) * bases[None, :].to(DEV)
    pe = torch.cat([torch.sin(arg), torch.cos(arg)], 1)
    lin = lambda x, w, b: x @ w.T + b
    pre = lin(pe, p[0], p[1]); sy0, saux0 = torch.sin(pre), torch.cos(pre)
    pre = lin(sy0, p[2], p[3]); sy1, saux1 = torch.sin(pre), torch.cos(pre)
    pre = lin(pe, p[4], p[5]); ty0, taux0 = torch.sin(pre), torch.cos(pre)
    pre = lin(ty0, p[6], p[7]); ty1, taux1 = torch.sin(pre), torch.cos(pre)
    hs = [torch.relu(lin(ty1, p[8 + 4 * i], p[9 + 4 * i])) for i in range(n)]
    outs = [lin(hs[i], p[10 + 4 * i], p[11 + 4 * i]) for i in range(n)]
    ctx = types.SimpleNamespace(n_mlp=n, B=B, pshapes=[tuple(t.shape) for t in flat],
                                saved_tensors=(pe, sy0, saux0, sy1, saux1, ty0, taux0, ty1, taux1, *hs, *outs, *[t.contiguous() for t in p]))
    before = dict(ops.TIME_BRANCH_BWD_CALLS)
    got = ops._TimeBranch.backward(ctx, *[c.to(DEV) for c in cots])
    after = ops.TIME_BRANCH_BWD_CALLS
    assert (after["taken"], after["declined"]) == (before["taken"], before["declined"] + 1), (before, after)
    assert got[:3] == (None, None, None)
    _within_bound(got[3:], ref, "declined")


def _tiny(B):
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    torch.manual_seed(1)
    model = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
    norm_idx = torch.tensor([(i + 1) / 7 for i in range(B)], dtype=torch.float64, device=DEV)
    frame = torch.rand(B, 3, 180, 320, generator=torch.Generator().manual_seed(3)).to(DEV)
    return model, norm_idx, frame


@pytest.mark.parametrize("B", [1, 2])
def test_tiny_model_gradients_and_captured_steps_equal_the_five_launch_form(B, monkeypatch):
    """The tiny NeRV_Boost at 180x320: forward, L1_freq loss, backward -- every parameter gradient bit-equal between the two forms; then
    three steps of the captured train step (one eager, the capture, a replay) from the same seed -- every parameter bit-equal."""
    from boosting_nerv_amd import hnerv_utils as hu
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adan
    grads, sds = {}, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BNERV_TIME_BRANCH_BWD", flag)
        model, norm_idx, frame = _tiny(B)
        before = ops.TIME_BRANCH_BWD_CALLS["taken"]
        img, _, _ = model(norm_idx, norm_idx=norm_idx)
        hu.loss_fn(img, frame, "L1_freq").backward()
        assert ops.TIME_BRANCH_BWD_CALLS["taken"] == before + (flag == "1"), "the tiny model's branch must be the kernels'"
        grads[flag] = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        model, norm_idx, frame = _tiny(B)
        opt = Adan(model.parameters(), lr=0.003)
        step = TrainStep(model, opt, "L1_freq", False, (B, 3, 180, 320), torch.device(DEV), use_graph=True, warmup_eager=1)
        for _ in range(3):
            step(frame, norm_idx)
        assert step.graph_a is not None
        sds[flag] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k in grads["1"]:
        assert torch.equal(grads["1"][k], grads["0"][k]), k
    for k in sds["1"]:
        assert torch.equal(sds["1"][k], sds["0"][k]), k
