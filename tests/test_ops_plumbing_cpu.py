"""Host-side plumbing of boosting_nerv_amd/ops.py without a device and without the library: WHICH C-ABI calls the convolution
operators issue, in which order, and where the deferred slab reductions are flushed.  A recording stand-in takes the place of the
loaded library, so the operators run on CPU tensors (whose contents are never computed: only the call sequence is checked)."""
import ctypes as C
import math

import pytest
import torch

QUERIES = ("_ws_bytes", "bnerv_conv_partial_rows", "bnerv_tanh_grad_blocks", "bnerv_cnx_mlp_plan", "bnerv_dwconv_wgrad_plan")      # answered on the host: no launch
PAIR, FLUSH = "bnerv_conv_wgrad_pair", "bnerv_flush_deferred"


def _ints(arg):
    """The non-pointer fields of a descriptor passed by reference."""
    d = getattr(arg, "_obj", None)
    if not isinstance(d, C.Structure):
        return None
    return tuple((n, getattr(d, n)) for n, t in d._fields_ if t is not C.c_void_p)


class RecordingLib:
    """Every bnerv_* entry point appends (name, integer fields of each descriptor argument) to `calls` and returns 0, except the
    sizes it is asked for: the split-K workspace (`splitk`), the other workspaces (64 bytes), the partial rows (2) -- and the pair
    launch, which answers `pair_rc` (0: taken, 1: not a pair the library takes)."""

    def __init__(self, pair_rc=0, splitk=0):
        self.pair_rc, self.splitk, self.calls = pair_rc, splitk, []

    def __getattr__(self, name):
        if not name.startswith("bnerv_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(i for i in map(_ints, args) if i is not None)))
            if name == "bnerv_conv_splitk_ws_bytes":
                return self.splitk
            if name.endswith("_ws_bytes"):
                return 64
            if name == "bnerv_conv_partial_rows":
                return 2
            if name == "bnerv_tanh_grad_blocks":
                return 1
            if name == "bnerv_last_error":
                return b""
            return self.pair_rc if name == PAIR else 0
        return fn

    def launches(self, start=0):
        return [n for n, _ in self.calls[start:] if not any(q in n for q in QUERIES)]


class Ctx:
    def __init__(self):
        self.handle, self.keep, self.dx_queued = None, [], False


@pytest.fixture
def rig(monkeypatch):
    """ops with the recording stand-in behind it: rig(pair_rc, splitk) -> (ops, lib, context)."""
    from boosting_nerv_amd import _lib as L, ops

    def make(pair_rc=0, splitk=0):
        lib, ctx = RecordingLib(pair_rc, splitk), Ctx()
        monkeypatch.setattr(L, "load", lambda optional=(): lib)
        monkeypatch.setattr(L, "stream", lambda: None)
        monkeypatch.setattr(L, "ctx", lambda create=True: ctx)
        monkeypatch.setattr(L, "require_device", lambda t, name="tensor": t)
        return ops, lib, ctx
    return make


# The smallest shapes the stem pair takes (csrc/stem.hip stem_dgrad_shape, bnerv_stem_pair_try): <= 256 pixels, >= 128 channels
# before the shuffle, <= 96 input channels.  A: x [1, 24, 4, 8] -> [1, 32, 8, 16]; B: 32 -> 128, shuffle 2 -> [1, 32, 16, 32].
def _p(*sh):
    return (torch.randn(*sh) / math.sqrt(sh[-1] * 9)).requires_grad_(True)


def _consumer(ops, kind, x):
    w, b = _p(128, 24, 3, 3), _p(128)
    if kind == "conv2d_ps":
        return ops.conv2d_ps(x, w, b, 2)
    if kind == "upconv_gelu":
        return ops.upconv_act(x, w, b, 2, "gelu")
    mods = [_p(1, 32, 1, 1) for _ in range(4)]
    return ops.snerv_block(x, w, b, *mods, _p(32, 32, 3, 3), _p(32), _p(32, 32, 3, 3), _p(32), 2)


def _chain_backward(ops, lib, kind, mode):
    """Forward of consumer A then conv2d_ps B, backward of both in `mode` (None: eager; else the dx_ok of lazy_flush).  Returns the
    launches of the backward alone and those issued when the lazy context closed."""
    x = torch.randn(1, 24, 4, 8).requires_grad_(True)
    out = ops.conv2d_ps(_consumer(ops, kind, x), _p(128, 32, 3, 3), _p(128), 2)
    assert out.shape == (1, 32, 16, 32)
    n0 = len(lib.calls)
    if mode is None:
        torch.autograd.grad(out, [x], torch.ones_like(out))
        return lib.launches(n0), []
    with ops.lazy_flush(dx_ok=mode):
        torch.autograd.grad(out, [x], torch.ones_like(out))
        bwd, n1 = lib.launches(n0), len(lib.calls)
    return bwd, lib.launches(n1)


KINDS = ["conv2d_ps", "snerv_block", "upconv_gelu"]


@pytest.mark.parametrize("kind", KINDS)
def test_a_queued_input_gradient_is_flushed_before_the_next_block_of_this_package_reads_it(rig, kind):
    """Block B's pair is the stem pair (taken, split-K slabs): its input gradient is a queued reduction.  Under lazy_flush(dx_ok=True)
    B does not flush -- so block A, which reads that gradient, must, before anything else it launches."""
    ops, lib, ctx = rig(pair_rc=0, splitk=64)
    bwd, tail = _chain_backward(ops, lib, kind, True)
    assert bwd[:2] == [PAIR, FLUSH], bwd                       # B's pair, then A's entry flush: nothing of A in between
    assert bwd.index(FLUSH) < bwd.index(PAIR, 1)
    assert bwd.count(FLUSH) == 1 and tail == [FLUSH]           # A's own queued dx waits for the context's closing flush
    assert not ctx.dx_queued and not ctx.keep


@pytest.mark.parametrize("mode", [None, False], ids=["eager", "lazy_dx_not_ok"])
@pytest.mark.parametrize("kind", KINDS)
def test_without_dx_ok_every_block_that_returns_a_queued_gradient_ends_with_its_own_flush(rig, kind, mode):
    ops, lib, ctx = rig(pair_rc=0, splitk=64)
    bwd, tail = _chain_backward(ops, lib, kind, mode)
    assert bwd[:2] == [PAIR, FLUSH] and bwd[-2:] == [PAIR, FLUSH], bwd
    assert bwd.count(FLUSH) == 2
    assert tail == ([] if mode is None else [FLUSH])
    assert not ctx.dx_queued and not ctx.keep


@pytest.mark.parametrize("dx_ok", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_queued_no_flush_inside_lazy_flush(rig, kind, dx_ok):
    """Same chain, no split-K workspace: no returned gradient is queued, so the entry line of a backward adds no launch."""
    ops, lib, ctx = rig(pair_rc=0, splitk=0)
    bwd, tail = _chain_backward(ops, lib, kind, dx_ok)
    assert FLUSH not in bwd and tail == [FLUSH], bwd


@pytest.mark.parametrize("dx_ok,flushes", [(True, 1), (False, 2)])
def test_stem_pair_block_fed_by_a_dense_layer_flushes_once_before_the_dense_backward(rig, dx_ok, flushes):
    """NeRV_Boost's arrangement: the stem MLP feeds the first block.  With dx_ok the block leaves its input gradient queued and the
    dense backward's entry flush is the only one; without, the block's own flush comes first."""
    ops, lib, ctx = rig(pair_rc=0, splitk=64)
    z = torch.randn(1, 16).requires_grad_(True)
    y, = ops.dense_grouped([z], [_p(24 * 4 * 8, 16)], [_p(24 * 4 * 8)], ["sin"])
    out = ops.conv2d_ps(y.view(1, 24, 4, 8), _p(128, 24, 3, 3), _p(128), 2)
    n0 = len(lib.calls)
    with ops.lazy_flush(dx_ok=dx_ok):
        torch.autograd.grad(out, [z], torch.ones_like(out))
    got = lib.launches(n0)
    assert got[:got.index("bnerv_dense_grouped_bwd") + 1] == [PAIR] + [FLUSH] * flushes + ["bnerv_dense_grouped_bwd"], got
    assert got[-1] == FLUSH and got.count(FLUSH) == flushes + 1


def test_pair_falls_back_to_the_two_launches_with_the_same_descriptors_and_leaves_its_arguments_alone(rig):
    ops, lib, ctx = rig(pair_rc=1, splitk=64)
    from boosting_nerv_amd import _lib as L
    x, g, w = torch.randn(1, 24, 4, 8), torch.randn(1, 32, 8, 16), torch.randn(128, 24, 3, 3)
    wg = dict(x=x, g=g, dw=torch.empty_like(w), db=torch.empty(128), B=1, Cin=24, Cout=128, H=4, W=8, k=3, in_mode=L.IN_PLAIN,
              g_mode=L.IN_UNSHUFFLE, g_s=2)
    cv = dict(x=g, w=w, bias=None, out=torch.empty_like(x), B=1, Cin=128, Cout=24, H=4, W=8, k=3, in_mode=L.IN_UNSHUFFLE,
              ep_mode=L.EP_PLAIN, in_s=2, transposed=1)
    wg0, cv0 = dict(wg), dict(cv)
    assert ops._wgrad_conv_pair(wg, cv) == (None, False)       # nothing reduced, and the fallback writes `out` directly
    assert wg == wg0 and cv == cv0                             # (same keys, the same tensor objects)
    assert lib.launches() == [PAIR, "bnerv_conv_wgrad", "bnerv_conv_igemm"]
    (_, (conv_i, wgrad_i)), (_, (wgrad_again,)), (_, (conv_again,)) = [c for c in lib.calls if c[0] in lib.launches()]
    assert wgrad_again == wgrad_i and conv_again == conv_i
    assert dict(conv_i)["Cin"] == 128 and dict(conv_i)["wCo"] == 128 and dict(conv_i)["wCi"] == 24 and dict(conv_i)["in_s"] == 2
    assert dict(wgrad_i)["defer_finish"] == 1 and dict(wgrad_i)["ws_bytes"] == 64 and dict(wgrad_i)["g_s"] == 2


def test_pair_taken_reports_a_queued_data_gradient_only_with_split_k_slabs(rig):
    from boosting_nerv_amd import _lib as L
    for splitk, queued in ((64, True), (0, False)):
        ops, lib, ctx = rig(pair_rc=0, splitk=splitk)
        x, g, w = torch.randn(1, 24, 4, 8), torch.randn(1, 32, 8, 16), torch.randn(128, 24, 3, 3)
        r = ops._wgrad_conv_pair(dict(x=x, g=g, dw=torch.empty_like(w), db=None, B=1, Cin=24, Cout=128, H=4, W=8, k=3, in_mode=L.IN_PLAIN,
                                      g_mode=L.IN_UNSHUFFLE, g_s=2),
                                 dict(x=g, w=w, bias=None, out=torch.empty_like(x), B=1, Cin=128, Cout=24, H=4, W=8, k=3,
                                      in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=2, transposed=1))
        assert r == (None, queued)
        assert lib.launches() == [PAIR] and len(ctx.keep) == 1 + queued      # the workspaces the queued jobs still read
        assert not ctx.dx_queued                                            # that is the block's to record, when it ends (ops._end_block)
