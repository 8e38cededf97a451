"""Global magnitude pruning on the device (csrc/prune.hip behind ops.kth_abs / prune_masks / mask_mul, optimizer.launch_grad_mask and
prune.Pruner): the select against torch.kthvalue bit for bit, the masks against torch.nn.utils.prune.global_unstructured and the CPU
Pruner, x *= mask at every alignment, and the masked train step -- captured replay against an eager step that masks its gradients with
stock torch -- with events between replays.

Every comparison of the kernels is exact (integer select, multiplications by 0 and 1).  The one tolerance, kept weights under an active
clip, is the bound tests/test_gpu_clip.py uses for a gradient scaled by the device clip (rtol 2e-6)."""
import copy
import glob
import math

import numpy as np
import pytest
import torch
import torch.nn.utils.prune as tprune

import hnerv_ref
from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

SHAPES = [(1,), (3,), (5, 7), (64, 3, 3, 3), (1031,), (300_001,)]
COUNTS = [int(np.prod(s)) for s in SHAPES]
N = sum(COUNTS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _at(values, k, pad=4):
    """`values` as a contiguous fp32 tensor k elements (4 k bytes) past a 16-byte boundary, NaN pads around it."""
    n = values.numel()
    buf = torch.full((n + 2 * pad,), NAN, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0 and k < pad
    v = buf[k:k + n]
    v.copy_(values.reshape(-1))
    assert v.data_ptr() % 16 == 4 * k
    return v.view(values.shape), buf


def _mask_at(values, j, pad=8):
    """uint8 `values` j bytes past a 16-byte boundary, pads of 7 around it."""
    n = values.numel()
    buf = torch.full((n + 2 * pad,), 7, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0 and j < pad
    v = buf[j:j + n]
    v.copy_(values.reshape(-1))
    return v.view(values.shape), buf


# ---------------------------------------------------------------------------------------------------------------------- select
def _values(case):
    g = torch.Generator().manual_seed(17)
    if case == "normal":
        x = torch.randn(N, generator=g) * 0.05
    elif case == "one_top_bin":                               # every magnitude in [0.5, 1): one bin of the top digit
        x = (0.5 + 0.5 * torch.rand(N, generator=g)).clamp(max=0.99999994) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
        assert x.abs().min() >= 0.5 and x.abs().max() < 1.0
    elif case == "lowest_digit":                              # bit patterns that differ in their lowest 8 bits only (and in sign)
        bits = 0x3F12AB00 + torch.randint(0, 256, (N,), generator=g, dtype=torch.int32)
        x = bits.view(torch.float32) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    elif case == "specials":                                  # +-0, denormals, +inf and pairs +-x among ordinary values
        x = torch.randn(N, generator=g)
        idx = torch.randperm(N, generator=g)
        x[idx[0:50]] = 0.0
        x[idx[50:100]] = -0.0
        x[idx[100:200]] = torch.randint(1, 5000, (100,), generator=g, dtype=torch.int32).view(torch.float32)      # denormals
        x[idx[200:230]] = -x[idx[100:130]]
        x[idx[230:240]] = float("inf")
        x[idx[240:1240]] = -x[idx[1240:2240]]               # pairs +-x
        x[0:4] = torch.tensor([float("inf"), -0.0, 1e-45, -1e-45])      # and in the tensors of one and three elements
    elif case == "zeros20":                                   # a fifth of the entries pruned already
        x = torch.randn(N, generator=g) * 0.1
        x[torch.rand(N, generator=g) < 0.2] = 0.0
    else:
        raise KeyError(case)
    return x.float()


_tables = {}


def _table(case):
    """The case's tensors on the device (every second one 4, 8 or 12 bytes past a 16-byte boundary) and their magnitudes on the host."""
    if case not in _tables:
        flat = _values(case)
        tensors, keep, at = [], [], 0
        for i, (shape, n) in enumerate(zip(SHAPES, COUNTS)):
            t, buf = _at(flat[at:at + n].to(DEV).view(shape), (i % 4) if i % 2 else (3 if i == 4 else 0))
            tensors.append(t); keep.append(buf)
            at += n
        assert tensors[1].data_ptr() % 16 == 4 and tensors[5].data_ptr() % 16 == 4 and tensors[3].data_ptr() % 16 == 12
        _tables[case] = (tensors, keep, flat.abs())
    return _tables[case]


KS = [1, 2, COUNTS[0] + COUNTS[1], sum(COUNTS[:3]), sum(COUNTS[:3]) + 1, sum(COUNTS[:5]), N // 2, N - 1, N]


@pytest.mark.parametrize("case", ["normal", "one_top_bin", "lowest_digit", "specials", "zeros20"])
def test_select_is_exact(case):
    from boosting_nerv_amd import ops
    tensors, _, mags = _table(case)
    got = [ops.kth_abs(tensors, k, return_flags=True) for k in KS] + [ops.kth_abs(tensors, KS[6], return_flags=True)]
    torch.cuda.synchronize()
    for k, (tau, n_pruned, flags) in zip(KS + [KS[6]], got):
        want = torch.kthvalue(mags, k).values
        count = int((mags <= want).sum())
        print(f"{case}: k {k}: tau {tau.item()!r} (kthvalue {want.item()!r}), pruned {n_pruned.item()} ((|w| <= tau).sum() {count})")
        assert tau.dtype == torch.float32 and n_pruned.dtype == torch.int64 and tau.is_cuda
        assert _bits(tau.cpu()).item() == _bits(want.reshape(1)).item(), (case, k)
        assert n_pruned.item() == count and count >= k, (case, k)
        assert flags.item() == 0, (case, k)
    assert torch.equal(_bits(got[6][0]), _bits(got[-1][0])) and torch.equal(got[6][1], got[-1][1])       # two runs, identical bits


def test_select_flags_a_nan_and_refuses_a_bad_rank():
    from boosting_nerv_amd import ops
    tensors, _, mags = _table("normal")
    for which, pos in ((0, 0), (4, 1030), (5, 299_999), (5, 123_457)):
        t = tensors[which].view(-1)
        old = t[pos].clone()
        t[pos] = NAN
        tau, n_pruned, flags = ops.kth_abs(tensors, 1000, return_flags=True)
        assert flags.item() & ops.KTH_FLAG_NAN, (which, pos)
        t[pos] = old
    assert ops.kth_abs(tensors, 1000, return_flags=True)[2].item() == 0
    for k in (0, N + 1, -3):
        with pytest.raises(ValueError):
            ops.kth_abs(tensors, k)


# ---------------------------------------------------------------------------------------------------------------------- masks
def _tiny(name, seed=3):
    from boosting_nerv_amd.model_hnerv import HNeRV
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    torch.manual_seed(seed)
    return NeRV_Boost(1, args=configs.tiny_nerv()) if name == "nerv" else HNeRV(hnerv_ref.tiny_args())


def _global_unstructured(model, k):
    from boosting_nerv_amd.prune import prunable
    twin = copy.deepcopy(model)
    names = [n for n, _ in prunable(model)]
    holders = []
    for n in names:
        mod, _, leaf = n.rpartition(".")
        holders.append((twin.get_submodule(mod) if mod else twin, leaf))
    tprune.global_unstructured(holders, pruning_method=tprune.L1Unstructured, amount=k)
    return {n: getattr(h, leaf + "_mask") for n, (h, leaf) in zip(names, holders)}


@pytest.mark.parametrize("name", ["nerv", "hnerv"])
def test_masks_equal_global_unstructured_and_the_cpu_pruner(name):
    from boosting_nerv_amd.prune import Pruner, prunable
    host = _tiny(name)
    before = {n: p.detach().clone() for n, p in host.named_parameters()}
    dev = copy.deepcopy(host).to(DEV)
    n = sum(p.numel() for _, p in prunable(host))
    cpu, gpu = Pruner(host), Pruner(dev)
    ptrs = {nm: m.data_ptr() for nm, m in gpu.masks.items()}
    for s in (0.3, 0.5):
        k = int(round(s * n))
        want = _global_unstructured(host, k)                 # (of the CURRENT weights: the zeros of the first event rank lowest)
        ev_h, ev_d = cpu.prune_to(s), gpu.prune_to(s)
        mags = torch.cat([before[nm].abs().reshape(-1) for nm, _ in prunable(host)])
        assert int((mags == ev_h["tau"]).sum()) == 1, "the weights tie at tau"
        assert ev_d == ev_h and ev_d["pruned"] == k, (ev_d, ev_h)
        for nm, p in prunable(dev):
            m = gpu.masks[nm].cpu()
            assert gpu.masks[nm].data_ptr() == ptrs[nm]                                 # the masks keep their addresses
            assert torch.equal(m.bool(), want[nm].bool()), (s, nm)
            assert torch.equal(m, cpu.masks[nm]), (s, nm)
            w = p.detach().cpu()
            assert torch.equal(_bits(w[m == 1]), _bits(before[nm][m == 1])), (s, nm)    # untouched where kept
            assert bool((w[m == 0] == 0).all()), (s, nm)                                # exactly zero where pruned
            assert torch.equal(w, dict(host.named_parameters())[nm].detach()), (s, nm)
        for nm, p in dev.named_parameters():
            if nm not in gpu.masks:
                assert torch.equal(p.detach().cpu(), before[nm]), nm
        assert abs(gpu.sparsity() - k / n) < 1e-12


def test_a_nan_in_the_prunable_set_raises_on_the_device():
    from boosting_nerv_amd.prune import Pruner, prunable
    model = _tiny("nerv").to(DEV)
    with torch.no_grad():
        prunable(model)[-1][1].view(-1)[5] = NAN
    with pytest.raises(ValueError, match="NaN"):
        Pruner(model).prune_to(0.2)


# ---------------------------------------------------------------------------------------------------------------------- x *= mask
_LENGTHS = list(range(1, 8)) + [4096 + t for t in range(8)] + [16384, 16385, 16384 * 2 + 3]


def _mul_items():
    g = torch.Generator().manual_seed(23)
    items = []
    for i, n in enumerate(_LENGTHS):
        for k in range(4):
            x = torch.randn(n, generator=g)
            x[::5] = -x[::5].abs()                            # (negative entries under a zero mask give -0)
            m = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
            xv, xbuf = _at(x.to(DEV), k)
            mv, mbuf = _mask_at(m.to(DEV), (i + 2 * k) % 8)
            items.append((xv, xbuf, mv, mbuf, x, m, k))
    return items


def _pads_intact(items, mask_written):
    for xv, xbuf, mv, mbuf, x, m, k in items:
        b = xbuf.cpu()
        assert torch.isnan(b[:k]).all() and torch.isnan(b[k + x.numel():]).all(), "a write outside the tensor"
        if mask_written:
            mb, j = mbuf.cpu(), mv.data_ptr() - mbuf.data_ptr()
            assert bool((mb[:j] == 7).all()) and bool((mb[j + m.numel():] == 7).all()), "a write outside the mask"


def test_mask_mul_at_unaligned_pointers_and_short_tails():
    from boosting_nerv_amd import ops
    items = _mul_items()
    assert {it[0].data_ptr() % 16 for it in items} == {0, 4, 8, 12} and len({it[2].data_ptr() % 4 for it in items}) == 4
    ops.mask_mul([it[0] for it in items], [it[2] for it in items])                       # ONE launch over the whole table
    torch.cuda.synchronize()
    for xv, xbuf, mv, mbuf, x, m, k in items:
        assert torch.equal(_bits(xv.cpu()), _bits(x * m.float())), (x.numel(), k)
        assert torch.equal(mv.cpu(), m)
    _pads_intact(items, False)


def test_prune_masks_at_unaligned_pointers_and_short_tails():
    from boosting_nerv_amd import ops
    items = _mul_items()
    tau = torch.tensor([0.6], device=DEV)
    for it in items:
        it[2].fill_(9)                                        # every mask byte is written
    ops.prune_masks([it[0] for it in items], [it[2] for it in items], tau)
    torch.cuda.synchronize()
    for xv, xbuf, mv, mbuf, x, m, k in items:
        keep = (x.abs() > 0.6000000238418579).to(torch.uint8)                             # (fp32 0.6)
        assert torch.equal(mv.cpu(), keep), (x.numel(), k)
        assert torch.equal(_bits(xv.cpu()), _bits(x * keep.float())), (x.numel(), k)
    _pads_intact(items, True)


def test_launch_grad_mask_over_the_optimizer_table():
    """Gradients of many sizes, some off the 16-byte grid, one above the 1024-block cap of a table entry (the grid-stride loop runs twice),
    a parameter without a mask and one without a gradient."""
    from boosting_nerv_amd.optimizer import Adan
    g = torch.Generator().manual_seed(29)
    sizes = [1, 3, 255, 256, 257, 1024, 4099, 2 ** 20 + 5] + [int(v) for v in torch.randint(1, 700, (40,), generator=g)]
    params, masks, want, bufs = [], {}, [], []
    for i, n in enumerate(sizes):
        p = torch.nn.Parameter(torch.zeros(n, device=DEV))
        vals = torch.randn(n, generator=g)
        k = (i % 3) + 1 if i % 2 else 0
        p.grad, buf = _at(vals.to(DEV), k)
        bufs.append((buf, k, n))
        if i % 5 != 4:
            m = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
            masks[p] = _mask_at(m.to(DEV), i % 4)[0]
            want.append(vals * m.float())
        else:
            want.append(vals)
        params.append(p)
    skipped = torch.nn.Parameter(torch.ones(37, device=DEV))
    opt = Adan(params[:5] + [skipped] + params[5:], lr=0.0)
    opt.set_grad_masks(masks)
    opt.launch_grad_mask()
    torch.cuda.synchronize()
    for p, w in zip(params, want):
        assert torch.equal(_bits(p.grad.cpu()), _bits(w)), p.numel()
    assert skipped.grad is None
    for buf, k, n in bufs:
        b = buf.cpu()
        assert torch.isnan(b[:k]).all() and torch.isnan(b[k + n:]).all(), "a write outside the gradient"


# ---------------------------------------------------------------------------------------------------------------------- the train step
_clip = {}


def _frames():
    from boosting_nerv_amd.synth import SyntheticVideo
    if "frames" not in _clip:
        vid = SyntheticVideo(3, 180, 320)
        _clip["frames"] = torch.stack([vid.frame(i) for i in range(3)]).to(DEV)
        _clip["norm"] = torch.tensor([(i + 1) / 3 for i in range(3)], dtype=torch.float64, device=DEV)
    return _clip["frames"], _clip["norm"]


def _build(name, clip_max_norm, masked, **kw):
    """(model, optimizer, pruner, step).  masked: the step under test, TrainStep(prune=pruner).  Otherwise its twin: TrainStep(prune=None)
    whose _clip_grads multiplies every gradient by its mask with stock torch first."""
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adam, Adan
    from boosting_nerv_amd.prune import Pruner, prunable
    model = _tiny(name, seed=1).to(DEV)
    opt = Adan(model.parameters(), lr=0.003) if name == "nerv" else Adam(model.parameters(), lr=0.003)
    pruner = Pruner(model, opt)

    class TorchMasked(TrainStep):
        def _clip_grads(self):
            for n, p in prunable(self.model):
                if p.grad is not None:
                    p.grad.mul_(pruner.masks[n].float())
            super()._clip_grads()
    loss, takes_image = ("Fusion10_freq", False) if name == "nerv" else ("L2", True)
    cls, extra = (TrainStep, dict(prune=pruner)) if masked else (TorchMasked, {})
    step = cls(model, opt, loss, takes_image, (1, 3, 180, 320), torch.device(DEV), clip_max_norm=clip_max_norm, **extra, **kw)
    return model, opt, pruner, step


def _pruned_are_zero(model, pruner):
    for n, p in model.named_parameters():
        if n in pruner.masks and not bool((p.detach()[pruner.masks[n] == 0] == 0).all()):
            return False
    return True


def _masked_trajectory(name, clip_max_norm, masked, **kw):
    frames, norm = _frames()
    model, opt, pruner, step = _build(name, clip_max_norm, masked, **kw)
    losses, events, graphs = [], [], []
    for s in range(8):
        if s in (0, 4):
            events.append(pruner.prune_to(0.3 if s == 0 else 0.5))
        loss, _ = step(frames[s % 3:s % 3 + 1], norm[s % 3:s % 3 + 1])
        losses.append(loss.item())
        graphs.append(step.graph_a)
        assert _pruned_are_zero(model, pruner), (name, s)
    # the optimizer state of a pruned weight is zero as well
    for n, p in model.named_parameters():
        if n in pruner.masks:
            for key, v in opt.state[p].items():
                if torch.is_tensor(v) and v.shape == p.shape:
                    assert bool((v[pruner.masks[n] == 0] == 0).all()), (n, key)
    return step, losses, events, graphs, {n: p.detach().clone() for n, p in model.named_parameters()}, pruner


@pytest.mark.parametrize("clip_max_norm", [0.0, 1.0])
@pytest.mark.parametrize("name", ["nerv", "hnerv"])
def test_masked_step_captured_equals_the_eager_step_masked_with_stock_torch(name, clip_max_norm):
    g_step, g_l, g_ev, g_graphs, g_w, g_pr = _masked_trajectory(name, clip_max_norm, True, use_graph=True, warmup_eager=2)
    e_step, e_l, e_ev, _, e_w, e_pr = _masked_trajectory(name, clip_max_norm, False, use_graph=False)
    assert g_step.prune is g_pr and e_step.prune is None and e_step.graph_a is None
    # steps 3.. were replays of ONE graph: the second event (in front of step 5) needed no re-capture
    assert g_graphs[0] is None and g_graphs[1] is None and g_graphs[2] is not None and all(g is g_graphs[2] for g in g_graphs[2:])
    assert g_ev == e_ev and g_ev[0]["pruned"] >= g_ev[0]["k"] > 0 and g_ev[1]["pruned"] >= g_ev[1]["k"] > g_ev[0]["pruned"]
    print(f"{name}, clip {clip_max_norm}: events {g_ev}, losses captured {g_l}, eager {e_l}")
    for n in g_pr.masks:
        assert torch.equal(g_pr.masks[n], e_pr.masks[n]), n
    if clip_max_norm == 0:
        assert g_l == e_l
        for n in g_w:
            assert torch.equal(g_w[n], e_w[n]), n
    else:
        for n in g_w:
            torch.testing.assert_close(g_w[n], e_w[n], rtol=2e-6, atol=0)
    # and the masks matter: an unpruned trajectory is another one
    assert abs(g_pr.sparsity() - 0.5) < 0.01


@pytest.mark.parametrize("name", ["nerv", "hnerv"])
def test_the_step_without_a_pruner_is_the_step_as_it_was(name):
    """TrainStep(prune=None) against the step's pieces driven by hand in the order they always had -- forward / backward, clip, schedule
    record, update -- from the same seed: the same parameters bit for bit, eager and captured; no mask launch, no mask pointers in the
    optimizer's tables.  A Pruner that has seen no event (masks all ones) changes no bit either."""
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adam, Adan
    from boosting_nerv_amd.prune import Pruner
    frames, norm = _frames()
    calls = []

    def run(mode):
        model = _tiny(name, seed=1).to(DEV)
        opt = Adan(model.parameters(), lr=0.003) if name == "nerv" else Adam(model.parameters(), lr=0.003)
        orig = opt.launch_grad_mask
        opt.launch_grad_mask = lambda: (calls.append(mode), orig())[1]
        loss, takes_image = ("Fusion10_freq", False) if name == "nerv" else ("L2", True)
        kw = dict(prune=Pruner(model, opt)) if mode == "ones" else {}
        step = TrainStep(model, opt, loss, takes_image, (1, 3, 180, 320), torch.device(DEV), clip_max_norm=1.0, use_graph=mode != "hand",
                         warmup_eager=2, **kw)
        losses = []
        for s in range(5):
            f, t = frames[s % 3:s % 3 + 1], norm[s % 3:s % 3 + 1]
            if mode == "hand":
                step.static_img.copy_(f); step.static_idx.copy_(t)
                step._fwd_bwd()
                opt.launch_clip(1.0)
                opt.prepare_step()
                opt.launch_step()
                losses.append(step.loss_out.item())
            else:
                losses.append(step(f, t)[0].item())
        if mode == "plain":
            assert step.prune is None and opt._grad_masks is None and step.graph_a is not None
        return losses, [p.detach().clone() for p in model.parameters()]
    hand, plain, ones = run("hand"), run("plain"), run("ones")
    assert "plain" not in calls and "hand" not in calls and calls.count("ones") >= 3
    assert hand[0] == plain[0] == ones[0], (hand[0], plain[0], ones[0])
    for a, b, c in zip(hand[1], plain[1], ones[1]):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------------- CLI
@pytest.mark.isolated
def test_cli_end_to_end(tmp_path, monkeypatch):
    """train_nerv_all.py on the tiny HNeRV baseline with two prune events, the .bnrq file of the pruned model, --eval_only from the
    checkpoint, and a second run from the same seed."""
    import re
    from PIL import Image
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    base = ("--data_path synthetic:4x180x320 --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none "
            "--crop_list 180_320 --resize_list -1 --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 "
            "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 --eval_freq 1 -p 2 -e 2 --prune_sparsity 0.4 --prune_steps 0 1")
    T.main((base + " --outf t --not_resume --dump_images --bitstream t.bnrq").split())
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    log = (out / "rank0.txt").read_text().splitlines()
    lines = [x for x in log if x.startswith("Prune: ")]
    assert len(lines) == 2, lines
    pat = re.compile(r"Prune: epoch (\d+), target ([0-9.]+), pruned (\d+) of (\d+) \(([0-9.]+)\), threshold ([0-9.e+-]+)")
    got = [pat.fullmatch(x).groups() for x in lines]
    n = int(got[0][3])
    for j, (epoch, target, pruned, n_, actual, tau) in enumerate(got):
        s = [1 - math.sqrt(0.6), 0.4][j]
        k = int(round(s * n))
        print(lines[j])
        assert int(epoch) == j and int(n_) == n and abs(float(target) - s) < 1e-4 and float(tau) > 0
        assert k <= int(pruned) <= k + 4 and abs(float(actual) - int(pruned) / n) < 1e-4           # up to ties at tau
    assert any(x.startswith("Train step: captured") for x in log)
    sparsity = [x for x in log if x.startswith("Sparsity: ")]
    assert len(sparsity) == 1 and f"{got[1][2]} of {n} " in sparsity[0]
    assert any("bits per parameter" in x for x in log[:log.index(sparsity[0])])
    # the checkpoint: masks and the zeros of the saved weights are the same thing
    ck = torch.load(out / "model_latest.pth", map_location="cpu")
    assert set(ck["prune"]) == {"masks", "shapes", "step_index"} and ck["prune"]["step_index"] == 1
    zeros = 0
    for name, packed in ck["prune"]["masks"].items():
        w = ck["state_dict"][name]
        assert not name.startswith("encoder.") and w.dim() > 1 and tuple(w.shape) == tuple(ck["prune"]["shapes"][name])
        m = torch.from_numpy(np.unpackbits(packed.numpy(), count=w.numel()).reshape(tuple(w.shape)))
        assert torch.equal(m == 0, w == 0), name
        zeros += int((m == 0).sum())
    assert zeros == int(got[1][2])
    # the file holds the pruned model: every decoded frame is the frame the quantised evaluation dumped
    dec = codec.Decoder(str(tmp_path / "t.bnrq"), DEV)
    assert len(dec) == 4
    for i in range(4):
        png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
        assert len(png) == 1, png
        assert np.array_equal(dec.decode_u8(i), np.asarray(Image.open(png[0]))), i
    # --eval_only from the checkpoint reports the same sparsity
    T.main((base + " --outf t --eval_only").split())
    again = [x for x in (out / "rank0.txt").read_text().splitlines() if x.startswith("Sparsity: ")]
    assert len(again) == 2 and again[1] == sparsity[0]
    # a run without the flags carries no trace of pruning; a second pruned run from the same seed repeats the masks bit for bit
    T.main((base + " --outf t2 --not_resume").split())
    ck2 = torch.load(tmp_path / "output" / "t2" / "tiny" / "Size0.05" / "model_latest.pth", map_location="cpu")
    for name, packed in ck["prune"]["masks"].items():
        assert torch.equal(packed, ck2["prune"]["masks"][name]), name
    T.main((base.replace(" -e 2 --prune_sparsity 0.4 --prune_steps 0 1", " -e 1") + " --outf t3 --not_resume").split())
    out3 = tmp_path / "output" / "t3" / "tiny" / "Size0.05"
    assert "prune" not in torch.load(out3 / "model_latest.pth", map_location="cpu")
    text3 = (out3 / "rank0.txt").read_text()
    assert "Prune:" not in text3 and "Sparsity:" not in text3
    # the generic eager step (stock torch.optim.Adam on a boost model) masks no gradient: refused before the first step
    nerv = ("--data_path synthetic:4x180x320 --vid tiny --model NeRV_Boost --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 --act sin "
            "--norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 --ks 0_3_3 --reduce 2 "
            "--dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 --lr 0.003 -e 1 --optim_type Adam --outf t4 --not_resume --prune_sparsity 0.3")
    with pytest.raises(NotImplementedError, match="captured train step"):
        T.main(nerv.split())
    assert "Epoch[" not in (tmp_path / "output" / "t4" / "tiny" / "Size0.05" / "rank0.txt").read_text()
