"""Global magnitude pruning, host side (no GPU): the flags of train_nerv_all, the schedule, the prunable set, and prune.Pruner on CPU
tensors -- the stock-torch restatement of the event that the GPU tests use as the oracle of csrc/prune.hip -- against
torch.nn.utils.prune.global_unstructured."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.utils.prune as tprune

import hnerv_ref
from conftest import ROOT
from oracle import configs

NEW_SYMBOLS = ("bnerv_kth_abs", "bnerv_prune_masks", "bnerv_mask_mul", "bnerv_grad_mask_table")


# ---------------------------------------------------------------------------------------------------------------------- library
def test_new_symbols_are_declared_bound_and_exported():
    from boosting_nerv_amd import _lib
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert C.sizeof(_lib.PruneItem) == 24 and _lib.PRUNE_SLICE == int(re.search(r"#define\s+BNERV_PRUNE_SLICE\s+(\d+)", header).group(1))


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(64)        # non-null, 16-byte aligned, never dereferenced: every call below fails its checks first
    assert lib.bnerv_kth_abs(None, None, None, 1, one, 1, 1, one) == -1 and b"kth_abs" in lib.bnerv_last_error()
    assert lib.bnerv_kth_abs(None, None, one, 0, one, 1, 1, one) == -1 and lib.bnerv_kth_abs(None, None, one, 1, one, 0, 1, one) == -1
    assert lib.bnerv_kth_abs(None, None, one, 1, one, 1, 0, one) == -1 and b"k=0" in lib.bnerv_last_error()
    assert lib.bnerv_kth_abs(None, None, one, 1, one, 1, 1, C.c_void_p(68)) == -1 and b"8-byte" in lib.bnerv_last_error()
    assert lib.bnerv_kth_abs(None, None, one, 1, one, 1, 1, one) == -1 and b"context missing" in lib.bnerv_last_error()      # no context: no scratch
    assert lib.bnerv_prune_masks(None, one, 1, one, 1, None) == -1 and b"prune_masks" in lib.bnerv_last_error()
    assert lib.bnerv_prune_masks(None, one, 1, C.c_void_p(66), 1, one) == -1 and b"aligned" in lib.bnerv_last_error()
    assert lib.bnerv_mask_mul(None, None, 1, one, 1) == -1 and b"mask_mul" in lib.bnerv_last_error()
    assert lib.bnerv_mask_mul(None, one, 1, one, 0) == -1
    assert lib.bnerv_grad_mask_table(None, one, 1, 1, None) == -1 and b"grad_mask_table" in lib.bnerv_last_error()
    assert lib.bnerv_grad_mask_table(None, one, 0, 1, one) == -1 and lib.bnerv_grad_mask_table(None, one, 1, 1, C.c_void_p(68)) == -1


def test_ops_raise_on_cpu_tensors():
    from boosting_nerv_amd import ops
    from boosting_nerv_amd._lib import BnervError
    w, m = torch.randn(5, 7), torch.ones(5, 7, dtype=torch.uint8)
    with pytest.raises(BnervError, match="no CPU fallback"):
        ops.kth_abs([w], 3)
    with pytest.raises(BnervError, match="no CPU fallback"):
        ops.prune_masks([w], [m], torch.zeros(1))
    with pytest.raises(BnervError, match="no CPU fallback"):
        ops.mask_mul([w], [m])


# ---------------------------------------------------------------------------------------------------------------------- flags, schedule
def test_parser_defaults_and_raises():
    from boosting_nerv_amd import train_nerv_all as T
    a = T.parse_args([])
    assert a.prune_sparsity == 0 and a.prune_steps == [0]
    a = T.parse_args("-e 5 --prune_sparsity 0.4 --prune_steps 3 0".split())
    assert a.prune_sparsity == 0.4 and a.prune_steps == [0, 3]
    for bad in ("--prune_sparsity 1.0", "--prune_sparsity -0.1", "--prune_sparsity 1.5", "--prune_sparsity nan",
                "-e 2 --prune_sparsity 0.3 --prune_steps 2", "-e 4 --prune_sparsity 0.3 --prune_steps 1 1", "-e 4 --prune_steps -1"):
        with pytest.raises(ValueError, match="prune_"):
            T.parse_args(bad.split())


def test_schedule_is_geometric_monotone_and_ends_at_S():
    from boosting_nerv_amd.prune import schedule
    ev = schedule(0.36, [0, 1])
    assert [e for e, _ in ev] == [0, 1] and abs(ev[0][1] - 0.2) < 1e-12 and ev[1][1] == 0.36
    ev = schedule(0.4, [7, 2])
    assert [e for e, _ in ev] == [2, 7] and abs(ev[0][1] - (1 - math.sqrt(0.6))) < 1e-12 and ev[1][1] == 0.4
    for S in (0.1, 0.5, 0.9):
        for m in (1, 3, 6):
            s = [x for _, x in schedule(S, range(m))]
            assert all(b > a for a, b in zip(s, s[1:])) and s[-1] == S and s[0] > 0
            # every event removes the same fraction of what is left
            left = [1.0] + [1 - x for x in s]
            ratios = [b / a for a, b in zip(left, left[1:])]
            assert max(ratios) - min(ratios) < 1e-12
    with pytest.raises(ValueError):
        schedule(1.0, [0])
    with pytest.raises(ValueError):
        schedule(0.5, [1, 1])


def _tiny(name):
    from boosting_nerv_amd.model_enerv import ENeRV_Boost
    from boosting_nerv_amd.model_hnerv import HNeRV, HNeRV_Boost
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    torch.manual_seed(3)
    return {"nerv": lambda: NeRV_Boost(1, args=configs.tiny_nerv()), "enerv": lambda: ENeRV_Boost(3, args=configs.tiny_enerv()),
            "hnerv": lambda: HNeRV(hnerv_ref.tiny_args()), "hnerv_boost": lambda: HNeRV_Boost(configs.tiny_hnerv())}[name]()


@pytest.mark.parametrize("name", ["nerv", "enerv", "hnerv", "hnerv_boost"])
def test_prunable_excludes_the_encoder_and_every_vector(name):
    from boosting_nerv_amd.prune import prunable
    model = _tiny(name)
    got = dict(prunable(model))
    assert got
    for n, p in model.named_parameters():
        want = p.dim() > 1 and not n.startswith("encoder.")
        assert (n in got) == want, n
        if want:
            assert got[n] is p
    assert not any(n.startswith("encoder.") for n in got) and all(p.dim() > 1 for p in got.values())
    if name in ("hnerv", "hnerv_boost"):
        assert any(n.startswith("encoder.") and p.dim() > 1 for n, p in model.named_parameters())      # there was something to exclude


# ---------------------------------------------------------------------------------------------------------------------- Pruner on the CPU
class Toy(torch.nn.Module):
    """Prunable shapes whose element counts are not multiples of 8, a bias, and an `encoder.` weight that must stay."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.encoder = torch.nn.Linear(6, 5)
        self.a = torch.nn.Parameter(torch.randn(5, 7, generator=g))
        self.b = torch.nn.Parameter(torch.randn(4, 3, 3, 3, generator=g))
        self.c = torch.nn.Parameter(torch.randn(1, 3, generator=g))
        self.bias = torch.nn.Parameter(torch.randn(13, generator=g))


def _global_unstructured(model, k):
    """The masks torch.nn.utils.prune gives a copy of the model's prunable set for amount=k."""
    import copy
    from boosting_nerv_amd.prune import prunable
    twin = copy.deepcopy(model)
    names = [n for n, _ in prunable(model)]
    holders = []
    for n in names:
        mod, _, leaf = n.rpartition(".")
        holders.append((twin.get_submodule(mod) if mod else twin, leaf))
    tprune.global_unstructured(holders, pruning_method=tprune.L1Unstructured, amount=k)
    return {n: getattr(h, leaf + "_mask") for n, (h, leaf) in zip(names, holders)}


@pytest.mark.parametrize("s", [0.1, 0.5, 0.93])
def test_cpu_pruner_equals_global_unstructured_on_tie_free_weights(s):
    from boosting_nerv_amd.prune import Pruner, prunable
    model = Toy()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    n = sum(p.numel() for _, p in prunable(model))
    assert n == 35 + 108 + 3
    k = int(round(s * n))
    want = _global_unstructured(model, k)
    pr = Pruner(model)
    ev = pr.prune_to(s)
    mags = torch.cat([before[nm].abs().reshape(-1) for nm, _ in prunable(model)])
    assert int((mags == ev["tau"]).sum()) == 1, "the weights tie at tau: global_unstructured's choice among ties is not defined"
    assert ev["k"] == k and ev["pruned"] == k and ev["n"] == n and ev["tau"] == float(torch.kthvalue(mags, k).values)
    for nm, p in prunable(model):
        assert torch.equal(pr.masks[nm].bool(), want[nm].bool()), nm
        assert torch.equal(p.detach(), before[nm] * want[nm]), nm
    for nm in ("bias", "encoder.weight", "encoder.bias"):
        assert torch.equal(dict(model.named_parameters())[nm].detach(), before[nm]), nm
    assert abs(pr.sparsity() - k / n) < 1e-12


def test_ties_at_tau_are_all_pruned_and_counted():
    from boosting_nerv_amd.prune import Pruner
    model = Toy()
    with torch.no_grad():
        model.a.copy_(torch.arange(1, 36, dtype=torch.float32).reshape(5, 7))
        model.b.fill_(100.0)
        model.c.copy_(torch.tensor([[-3.0, 3.0, 0.5]]))
    pr = Pruner(model)
    ev = pr.prune_to(3 / 146)                     # k = 3: 0.5, 1, 2 ... but rank 3 may not split the four entries of magnitude 3
    assert ev["k"] == 3 and ev["tau"] == 2.0 and ev["pruned"] == 3
    ev = pr.prune_to(4 / 146)                     # k = 4 lands on |w| = 3, held by a[0, 2], c[0, 0] and c[0, 1]
    assert ev["k"] == 4 and ev["tau"] == 3.0 and ev["pruned"] == 6
    assert model.c.detach().abs().sum() == 0 and pr.masks["c"].sum() == 0
    assert model.a.detach().reshape(-1)[:4].tolist() == [0.0, 0.0, 0.0, 4.0]
    assert abs(pr.sparsity() - 6 / 146) < 1e-12


def test_masks_are_nested_over_two_events_and_k_zero_changes_nothing():
    from boosting_nerv_amd.prune import Pruner
    model = Toy(1)
    pr = Pruner(model)
    w0 = model.a.detach().clone()
    ev = pr.prune_to(0.001)                       # k = round(0.146) = 0
    assert ev == {"k": 0, "pruned": 0, "n": 146, "tau": 0.0} and torch.equal(model.a.detach(), w0) and pr.sparsity() == 0.0
    pr.prune_to(0.3)
    first = {n: m.clone() for n, m in pr.masks.items()}
    ev = pr.prune_to(0.5)
    assert ev["pruned"] == ev["k"] == 73
    for n, m in pr.masks.items():
        assert bool(((m == 1) <= (first[n] == 1)).all()), n          # kept now => kept before
    assert sum(int((first[n] - m).sum()) for n, m in pr.masks.items()) == 73 - 44


def test_state_dict_round_trip_with_counts_that_are_no_multiple_of_eight():
    from boosting_nerv_amd.prune import Pruner
    model = Toy(2)
    pr = Pruner(model)
    pr.prune_to(0.4)
    pr.step_index = 1
    sd = pr.state_dict()
    assert sd["shapes"] == {"a": (5, 7), "b": (4, 3, 3, 3), "c": (1, 3)} and sd["step_index"] == 1
    assert sd["masks"]["a"].dtype == torch.uint8 and sd["masks"]["a"].numel() == 5 and sd["masks"]["b"].numel() == 14 and sd["masks"]["c"].numel() == 1
    assert np.array_equal(sd["masks"]["a"].numpy(), np.packbits(pr.masks["a"].numpy().reshape(-1)))
    import io
    buf = io.BytesIO()
    torch.save({"prune": sd}, buf)
    buf.seek(0)
    back = Pruner(Toy(2))
    ptrs = {n: m.data_ptr() for n, m in back.masks.items()}
    back.load_state_dict(torch.load(buf, map_location="cpu")["prune"])
    assert back.step_index == 1 and back.sparsity() == pr.sparsity()
    for n, m in pr.masks.items():
        assert torch.equal(back.masks[n], m) and back.masks[n].data_ptr() == ptrs[n], n      # restored into the tensors that exist
    other = torch.nn.Sequential(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError):
        Pruner(other).load_state_dict(sd)


def test_a_nan_in_the_prunable_set_raises_and_one_outside_does_not():
    from boosting_nerv_amd.prune import Pruner
    model = Toy(3)
    with torch.no_grad():
        model.bias[0] = float("nan")
        model.encoder.weight[0, 0] = float("nan")
    Pruner(model).prune_to(0.2)
    with torch.no_grad():
        model.b[1, 2, 0, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        Pruner(model).prune_to(0.2)


@pytest.mark.parametrize("kind", ["adam", "adan"])
def test_optimizer_state_is_masked_at_an_event(kind):
    """A toy optimizer state of torch.optim.Adam's / Adan's layout: every per-element tensor of a prunable parameter is multiplied by the
    mask (Adan's previous gradient included), the step counter and the state of other parameters are not touched."""
    from boosting_nerv_amd.prune import Pruner
    model = Toy(4)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)            # a holder for .state: the event only reads optimizer.state
    keys = ["exp_avg", "exp_avg_sq"] + (["exp_avg_diff", "neg_pre_grad"] if kind == "adan" else [])
    g = torch.Generator().manual_seed(5)
    for p in model.parameters():
        opt.state[p] = {k: torch.randn(p.shape, generator=g) + 3.0 for k in keys}
        if kind == "adam":
            opt.state[p]["step"] = torch.tensor(7.0)
    before = {p: {k: v.clone() for k, v in st.items()} for p, st in opt.state.items()}
    pr = Pruner(model, opt)
    ev = pr.prune_to(0.5)
    assert ev["pruned"] == 73
    masks = {id(dict(model.named_parameters())[n]): m for n, m in pr.masks.items()}
    for p, st in opt.state.items():
        for k in keys:
            want = before[p][k] * masks[id(p)] if id(p) in masks else before[p][k]
            assert torch.equal(st[k], want), k
        if kind == "adam":
            assert st["step"].item() == 7.0


def test_compression_step_and_foreign_steps_refuse_a_pruner():
    from boosting_nerv_amd import engine
    import inspect
    assert inspect.signature(engine.TrainStep.__init__).parameters["prune"].default is None
    with pytest.raises(NotImplementedError, match="plain train step"):
        engine.CompressionStep(None, None, None, None, None, None, prune=object())
