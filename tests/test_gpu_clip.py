"""Global-norm gradient clipping on the device (bnerv_grad_sqsum_table + bnerv_grad_scale_table behind optimizer.launch_clip) against
torch.nn.utils.clip_grad_norm_'s definition evaluated in float64, and the train step that holds it: eager and captured steps with an
active clip agree bit for bit, with and without the flat gradient bucket.

Tolerances: the sum of squares is accumulated in float64, so clip_out[0] carries one fp32 rounding of the square root (rtol 1e-6); a scaled
gradient carries the fp32 roundings of the coefficient (norm, + 1e-6, division) and one of the product (rtol 2e-6)."""
import os

import numpy as np
import pytest
import torch

from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

_rng = np.random.RandomState(7)
SETS = {
    "one": [1],
    "edges": [3, 255, 256, 257, 1024, 4099],
    "many": [int(n) for n in _rng.randint(1, 700, size=200)],
    "big": [2 ** 20 + 5],           # 1025 chunks of 1024 elements on the 1024-block cap: the grid-stride loop runs more than once
}


def _grad_at(values, k):
    """The values as a contiguous fp32 tensor k elements (4 k bytes) past a 16-byte boundary, NaN pads around it (tests/test_gpu_alignment.py)."""
    n = values.numel()
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf.fill_(NAN)
    v = buf[k:k + n]
    v.copy_(values)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
    return v, buf


def _make(sizes, zero=False):
    """Parameters with gradients of the given sizes; the last one, and every seventh, sits 4 (8, 12) bytes past a 16-byte boundary; one extra
    parameter in the middle has no gradient.  -> (optimizer, parameters with a gradient, their float64 gradients, the padded buffers)."""
    from boosting_nerv_amd.optimizer import Adan
    g = torch.Generator().manual_seed(11)
    params, bufs = [], []
    for i, n in enumerate(sizes):
        p = torch.nn.Parameter(torch.zeros(n, device=DEV))
        vals = torch.zeros(n) if zero else torch.randn(n, generator=g) * (0.01 + 0.1 * (i % 5))
        k = 1 if i == len(sizes) - 1 else ((i // 7) % 3 + 1 if i % 7 == 6 else 0)
        if k:
            p.grad, buf = _grad_at(vals.to(DEV), k)
            bufs.append((buf, k, n))
        else:
            p.grad = vals.to(DEV)
            assert p.grad.data_ptr() % 16 == 0
        params.append(p)
    skipped = torch.nn.Parameter(torch.ones(37, device=DEV))          # grad is None: not part of the norm, not touched
    allp = params[:len(params) // 2] + [skipped] + params[len(params) // 2:]
    opt = Adan(allp, lr=0.0)
    ref = [p.grad.detach().cpu().double().numpy().copy() for p in params]
    return opt, params, ref, bufs, skipped


def _pads_intact(bufs):
    for buf, k, n in bufs:
        b = buf.cpu()
        assert torch.isnan(b[:k]).all() and torch.isnan(b[k + n:]).all(), "a write outside the gradient"


@pytest.mark.parametrize("regime", ["inactive", "active", "zero"])
@pytest.mark.parametrize("name", list(SETS))
def test_launch_clip_against_clip_grad_norm_semantics_in_float64(name, regime):
    sizes = SETS[name]
    opt, params, ref, bufs, skipped = _make(sizes, zero=regime == "zero")
    assert any(k == 1 for _, k, _ in bufs)                             # one gradient 4 bytes past a 16-byte boundary
    total = float(np.sqrt(sum(float((g * g).sum()) for g in ref)))
    max_norm = {"inactive": 2.0 * total, "active": 0.5 * total, "zero": 1.0}[regime]
    coef = min(1.0, max_norm / (total + 1e-6))
    before = [p.grad.detach().clone() for p in params]
    opt.launch_clip(max_norm)
    torch.cuda.synchronize()
    out = opt.clip_out.cpu().numpy()
    print(f"{name}/{regime}: total {out[0]!r} (float64 {total!r}), coef {out[1]!r} (float64 {coef!r})")
    np.testing.assert_allclose(out[0], total, rtol=1e-6, atol=0)
    if regime == "active":
        assert out[1] < 1.0
        np.testing.assert_allclose(out[1], coef, rtol=1e-6, atol=0)
        for p, g in zip(params, ref):
            np.testing.assert_allclose(p.grad.cpu().numpy(), g * coef, rtol=2e-6, atol=0)
    else:
        assert out[1] == 1.0 and coef == 1.0                           # exactly one: the gradients keep their bits
        for p, b in zip(params, before):
            assert torch.equal(p.grad, b)
    assert skipped.grad is None
    _pads_intact(bufs)


@pytest.mark.parametrize("name", ["edges", "many", "big"])
def test_launch_clip_is_bitwise_reproducible(name):
    res = []
    for _ in range(2):
        opt, params, ref, bufs, _ = _make(SETS[name])
        total = float(np.sqrt(sum(float((g * g).sum()) for g in ref)))
        opt.launch_clip(0.5 * total)
        opt.launch_clip(0.125 * total)                                 # a second clip over the same table: half of the first one's result
        torch.cuda.synchronize()
        res.append(([p.grad.detach().clone() for p in params], opt.clip_out.clone()))
    assert torch.equal(res[0][1], res[1][1])
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)


# ---- the train step -----------------------------------------------------------------------------------------------------------------
_clip = {}


def _frames():
    from boosting_nerv_amd.synth import SyntheticVideo
    if "frames" not in _clip:
        vid = SyntheticVideo(3, 180, 320)
        _clip["frames"] = torch.stack([vid.frame(i) for i in range(3)]).to(DEV)
        _clip["norm"] = torch.tensor([(i + 1) / 3 for i in range(3)], dtype=torch.float64, device=DEV)
    return _clip["frames"], _clip["norm"]


def _step(clip_max_norm, lr=0.003, **kw):
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    from boosting_nerv_amd.optimizer import Adan
    torch.manual_seed(1)
    model = NeRV_Boost(1, args=configs.tiny_nerv()).to(DEV)
    opt = Adan(model.parameters(), lr=lr)
    return model, opt, TrainStep(model, opt, "Fusion10_freq", False, (1, 3, 180, 320), torch.device(DEV), clip_max_norm=clip_max_norm, **kw)


def _first_norm():
    """Gradient norm of the first step (eager, parameters frozen by lr = 0), in float64."""
    if "norm0" not in _clip:
        frames, norm = _frames()
        model, opt, step = _step(0.0, lr=0.0, use_graph=False)
        step(frames[0:1], norm[0:1])
        _clip["norm0"] = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in model.parameters() if p.grad is not None)))
    return _clip["norm0"]


def _trajectory(clip_max_norm, n=6, **kw):
    frames, norm = _frames()
    model, opt, step = _step(clip_max_norm, **kw)
    losses, psnrs, coefs = [], [], []
    for s in range(n):
        loss, psnr = step(frames[s % 3:s % 3 + 1], norm[s % 3:s % 3 + 1])
        losses.append(loss.item()); psnrs.append(psnr.item()); coefs.append(opt.clip_out[1].item() if clip_max_norm > 0 else None)
    return step, losses, psnrs, coefs, [p.detach().clone() for p in model.parameters()]


def test_clipped_step_eager_and_captured_agree_bit_for_bit():
    max_norm = 0.5 * _first_norm()
    e_step, e_l, e_p, e_c, e_w = _trajectory(max_norm, use_graph=False)
    g_step, g_l, g_p, g_c, g_w = _trajectory(max_norm, use_graph=True, warmup_eager=2)
    assert e_step.graph_a is None and g_step.use_graph and g_step.graph_a is not None      # a clip no longer costs the graph
    assert e_c[0] < 1.0 and g_c[0] < 1.0, (e_c, g_c)                                         # the clip is active
    assert e_l == g_l and e_p == g_p and e_c == g_c, (e_l, g_l, e_c, g_c)
    for a, b in zip(e_w, g_w):
        assert torch.equal(a, b)
    # and it matters: the unclipped trajectory is another one
    _, u_l, _, _, _ = _trajectory(0.0, use_graph=False, n=3)
    assert u_l[0] == e_l[0] and u_l[1:] != e_l[1:3]


def test_clipped_step_gradients_against_clip_grad_norm():
    """One step from identical state, parameters frozen by Adan's lr = 0 so that .grad survives the step: the post-clip gradients against
    torch.nn.utils.clip_grad_norm_ applied to copies of the unclipped ones."""
    frames, norm = _frames()
    max_norm = 0.5 * _first_norm()
    model, opt, step = _step(0.0, lr=0.0, use_graph=False)
    step(frames[0:1], norm[0:1])
    copies = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    for c, p in zip(copies, model.parameters()):
        c.grad = p.grad.detach().clone()
    total = torch.nn.utils.clip_grad_norm_(copies, max_norm)
    model2, opt2, step2 = _step(max_norm, lr=0.0, use_graph=False)
    step2(frames[0:1], norm[0:1])
    assert opt2.clip_out[1].item() < 1.0
    print(f"total norm: device {opt2.clip_out[0].item()!r}, clip_grad_norm_ (fp32 sums) {total.item()!r}")
    for c, p in zip(copies, model2.parameters()):
        torch.testing.assert_close(p.grad, c.grad, rtol=2e-6, atol=0)


@pytest.mark.isolated
def test_clipped_step_with_the_flat_bucket_on_one_rank_equals_the_step_without():
    """force_bucket on a 1-rank RCCL group (gather -> all-reduce -> scatter -> clip -> Adan; one graph with the collective inside, and
    graph A -> eager all-reduce -> graph B): the mean over one rank is the identity, so the clipped trajectory is the plain one's."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29617")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        max_norm = 0.5 * _first_norm()
        _, l0, p0, c0, w0 = _trajectory(max_norm, use_graph=True, warmup_eager=2)
        assert c0[0] < 1.0
        for ingraph in ("1", "0"):
            os.environ["BNERV_DP_INGRAPH"] = ingraph
            step, l1, p1, c1, w1 = _trajectory(max_norm, use_graph=True, warmup_eager=2, force_bucket=True)
            assert step.graph_a is not None and (ingraph == "1" or step.graph_b is not None)
            assert l1 == l0 and p1 == p0 and c1 == c0, (ingraph, l0, l1, c0, c1)
            for a, b in zip(w0, w1):
                assert torch.equal(a, b)
        os.environ.pop("BNERV_DP_INGRAPH", None)
    finally:
        if created:
            dist.destroy_process_group()
