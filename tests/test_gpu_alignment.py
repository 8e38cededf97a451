"""GPU tests (``-m gpu``) of every operator on operands that are NOT 16-byte aligned.

The caching allocator hands out 512-byte aligned blocks, so the rest of the suite only ever passes aligned pointers; pointer alignment is
a dispatch input across the library (csrc/launch.h conv_vec_ok, the `vec` flags of wgrad.hip / eltwise.hip / dwconv.hip, INTEGRATION.md
"Pointer alignment").  Here the operands are contiguous fp32 views at data_ptr % 16 == 4 k (a slice of a flat buffer, a split of a flat
parameter vector, a frame of a clip with an odd frame size), at shapes with W % 4 == 0 where an aligned call takes a vector path.

Every case computes (a) the float64 stock-torch reference on the CPU (the expressions of test_gpu_ops / test_gpu_hnerv /
test_gpu_ssim_loss), (b) the operator on aligned copies, (c) the operator with some operands shifted, and asserts (c) against (a) and
(c) against (b) with that operator's existing comparison (close() of test_gpu_ops -- SURVEY 8(d) -- or the loss tests' 2e-4 / 2e-3
forms).  Where the remedy is an aligned copy, or where no kernel of the operator looks at alignment, (c) must equal (b) bit for bit --
provided (b) run twice gives the same bits; otherwise that case falls back to close()."""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref, msssim_ref
from test_gpu_hnerv import _ref_upconv
from test_gpu_ops import _tat_inputs, _tat_ref, close, gpu
from test_gpu_ssim_loss import loss_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


def shifted(t, k):
    """Same values, contiguous, k elements past a 16-byte boundary (fp32: data_ptr % 16 == 4 k, k in 1..3), with NaN pads on both sides.
    Returns (the detached view, requires_grad copied; the whole buffer)."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf.fill_(NAN)
    v = buf[k:k + n].view(t.shape)
    v.copy_(t.detach())
    return v.detach().requires_grad_(t.requires_grad), buf


def check_shifted(v, k):
    """The three facts without which a test here would pass vacuously."""
    from boosting_nerv_amd import _lib as L
    assert v.is_contiguous()
    assert v.data_ptr() % 16 == (k * v.element_size()) % 16 != 0
    assert L.f32c(v).data_ptr() == v.data_ptr() or v.dtype != torch.float32


def pads_intact(buf, k):
    n = buf.numel() - 4
    return bool(torch.isnan(buf[:k]).all()) and bool(torch.isnan(buf[k + n:]).all())


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# the generic (a) / (b) / (c) harness for autograd operators
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """make() -> (fp32 CPU leaves with requires_grad, cotangent); ref(*float64 leaves) -> output; run(ops, *device leaves) -> output;
    names: one per leaf; exact: (c) must equal (b) bit for bit; env: environment switches; ctx: context manager around the backward."""

    def __init__(self, key, make, ref, run, names, exact=False, env=None, ctx=None):
        self.key, self.make, self.ref, self.run, self.names, self.exact, self.env, self.ctx = key, make, ref, run, names, exact, env or {}, ctx

    def backward_ctx(self, ops):
        return self.ctx(ops) if self.ctx else contextlib.nullcontext()


_BASE = {}


def _baseline(case, ops):
    """(a) and (b) of a case, computed once and shared by its variants (never modified afterwards)."""
    if case.key not in _BASE:
        leaves, cot = case.make()
        ld = [t.detach().double().requires_grad_(True) for t in leaves]
        ref = case.ref(*ld)
        rg = torch.autograd.grad(ref, ld, cot.double())
        runs = []
        for _ in range(2):
            gl = [gpu(t) for t in leaves]
            out = case.run(ops, *gl)
            with case.backward_ctx(ops):
                gg = torch.autograd.grad(out, gl, cot.to(DEV))
            runs.append([out.detach()] + [g.detach() for g in gg])
        det = all(same(x, y) for x, y in zip(*runs))
        print(f"{case.key}: the aligned call gives the same bits twice: {det}")
        for n, x, r in zip(["fwd"] + ["d" + n for n in case.names], runs[0], [ref] + list(rg)):
            close(x, r.float(), msg=f"{case.key} aligned {n}")
        _BASE[case.key] = (leaves, cot, [ref.detach().float()] + [g.float() for g in rg], runs[0], det)
    return _BASE[case.key]


def run_variant(case, ops, which, k, monkeypatch):
    """which: 'x' (the activation input alone), 'cot' (the cotangent alone), 'all' (everything the caller supplies), or a leaf name."""
    for name, val in case.env.items():
        monkeypatch.setenv(name, val)
    leaves, cot, refs, base, det = _baseline(case, ops)
    idx = {"x": {0}, "cot": set(), "all": set(range(len(leaves)))}.get(which)
    if idx is None:
        idx = {case.names.index(which)}
    gl, bufs = [], []
    for i, t in enumerate(leaves):
        v = gpu(t)
        if i in idx:
            v, buf = shifted(v, k)
            check_shifted(v, k)
            bufs.append((v, buf, t))
        gl.append(v)
    cs = cot.to(DEV)
    if which in ("cot", "all"):
        cs, cbuf = shifted(cs, k)
        check_shifted(cs, k)
        bufs.append((cs, cbuf, cot))
    out = case.run(ops, *gl)
    seen = []
    out.register_hook(lambda g: seen.append(g.data_ptr()))
    with case.backward_ctx(ops):
        gg = torch.autograd.grad(out, gl, cs)
    assert seen == [cs.data_ptr()], "the operator's backward did not receive the cotangent at the address the test chose"
    got = [out] + list(gg)
    tags = ["fwd"] + ["d" + n for n in case.names]
    for n, x, r in zip(tags, got, refs):
        assert torch.isfinite(x).all(), f"{case.key} [{which} +{4 * k}B] {n}: non-finite"
        close(x, r, msg=f"{case.key} [{which} +{4 * k}B] {n} vs float64")
    for n, x, b in zip(tags, got, base):
        if case.exact and det:
            assert same(x, b), f"{case.key} [{which} +{4 * k}B] {n}: differs from the aligned call, max {float((x - b).abs().max()):.3e}"
        else:       # another kernel family (or a result that is not reproducible call to call): the operator's own tolerance
            close(x, b, msg=f"{case.key} [{which} +{4 * k}B] {n} vs aligned")
    for v, buf, t in bufs:                                  # inputs are inputs: values and guard elements untouched
        assert pads_intact(buf, k) and torch.equal(v.detach().cpu(), t.detach()), f"{case.key} [{which}]: an input buffer was written"


VARIANTS = [("x", 1), ("cot", 1), ("all", 1), ("x", 2), ("cot", 2), ("all", 2)]
VIDS = [f"{w}+{4 * k}B" for w, k in VARIANTS]


def _sid(shape):
    return "-".join(str(v) for v in shape)


# ---------------------------------------------------------------------------------------------------------------- conv2d_ps
def conv_case(shape, lazy=False):
    B, Cin, Ct, H, W, k, s = shape

    def make():
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(B, Cin, H, W, generator=g).requires_grad_(True)
        w = (torch.randn(Ct, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).requires_grad_(True)
        b = torch.randn(Ct, generator=g).requires_grad_(True)
        return [x, w, b], torch.randn(B, Ct // (s * s), H * s, W * s, generator=g)
    return Case(f"conv2d_ps {_sid(shape)}{' lazy' if lazy else ''}", make, lambda x, w, b: cpu_ref.upconv(x, w, b, s),
                lambda ops, x, w, b: ops.conv2d_ps(x, w, b, s), ["x", "w", "b"], ctx=(lambda ops: ops.lazy_flush(dx_ok=False)) if lazy else None)


CONV_SHAPES = [
    (1, 12, 12, 16, 64, 3, 1),       # conv4 family
    (1, 38, 38, 24, 64, 3, 1),       # wide split
    (1, 40, 160, 16, 32, 3, 2), (1, 20, 180, 24, 36, 3, 3), (1, 24, 400, 9, 16, 3, 5),     # PixelShuffle 2 / 3 / 5 gathers
    (2, 30, 750, 9, 16, 3, 5),       # low-resolution family
    (2, 79, 594, 9, 16, 3, 3),       # stem pair
    (1, 95, 100, 9, 16, 1, 5),       # k = 1
    (1, 48, 20, 64, 68, 1, 1),       # k = 1 from 4096 pixels on: wgrad1.hip
]
CONV_CASES = [conv_case(s) for s in CONV_SHAPES] + [conv_case((2, 79, 594, 9, 16, 3, 3), lazy=True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.key.replace(" ", "_"))
def test_conv2d_ps(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- TAT / SNeRV blocks
TAT_NAMES = ["x0", "s0", "t0", "s1", "t1", "w0", "b0", "w1", "b1"]


def tat_case(shape, seed=7, env=None, tag=""):
    def make():
        x0, mods, w0, b0, w1, b1, g = _tat_inputs(*shape, seed=seed)
        return [x0] + mods + [w0, b0, w1, b1], torch.randn(x0.shape, generator=g)
    return Case(f"tat_block {_sid(shape)}{tag}", make, lambda x0, s0, t0, s1, t1, w0, b0, w1, b1: _tat_ref(x0, [s0, t0, s1, t1], w0, b0, w1, b1),
                lambda ops, *gl: ops.tat_block(*gl), TAT_NAMES, env=env)


TAT_CASES = [tat_case(s) for s in [(1, 12, 16, 64), (2, 38, 9, 40), (1, 95, 9, 16), (1, 30, 45, 80)]] + [
    # the shared-tile pair forced on: its fold form (wgrad.hip launch_pair) and the transforming form
    tat_case((1, 12, 48, 96), seed=31, env={"BNERV_PAIR_FUSED": "8", "BNERV_PAIR_FOLD": "1"}, tag=" fold"),
    tat_case((1, 12, 48, 96), seed=31, env={"BNERV_PAIR_FUSED": "8", "BNERV_PAIR_FOLD": "0"}, tag=" transform"),
]


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", TAT_CASES, ids=lambda c: c.key.replace(" ", "_"))
def test_tat_block(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


def snerv_case(shape):
    B, Cin, Cc, H, W, k, s = shape

    def make():
        x0, mods, w0, b0, w1, b1, g = _tat_inputs(B, Cc, H * s, W * s, seed=11)
        x = torch.randn(B, Cin, H, W, generator=g).requires_grad_(True)
        wu = (torch.randn(Cc * s * s, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).requires_grad_(True)
        bu = (torch.randn(Cc * s * s, generator=g) * 0.1).requires_grad_(True)
        return [x, wu, bu] + mods + [w0, b0, w1, b1], torch.randn(x0.shape, generator=g)
    return Case(f"snerv_block {_sid(shape)}", make,
                lambda x, wu, bu, s0, t0, s1, t1, w0, b0, w1, b1: _tat_ref(torch.sin(cpu_ref.upconv(x, wu, bu, s)), [s0, t0, s1, t1], w0, b0, w1, b1),
                lambda ops, *gl: ops.snerv_block(*gl, s), ["x", "wu", "bu"] + TAT_NAMES[1:])


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", [snerv_case(s) for s in [(1, 12, 12, 16, 64, 3, 1), (1, 40, 38, 16, 32, 3, 2), (1, 20, 20, 24, 36, 3, 3)]],
                         ids=lambda c: c.key.replace(" ", "_"))
def test_snerv_block(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- head + tanh
def head_case(shape, k, env=None, tag=""):
    B, Cin, Cout, H, W = shape

    def make():
        g = torch.Generator().manual_seed(sum(shape) + k)
        x = torch.randn(B, Cin, H, W, generator=g).requires_grad_(True)
        w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).requires_grad_(True)
        b = torch.randn(Cout, generator=g).requires_grad_(True)
        return [x, w, b], torch.randn(B, Cout, H, W, generator=g)
    return Case(f"head_tanh k{k} {_sid(shape)}{tag}", make, lambda x, w, b: cpu_ref.out_img(F.conv2d(x, w, b, padding=(k - 1) // 2)),
                lambda ops, x, w, b: ops.head_tanh(x, w, b), ["x", "w", "b"], env=env)


HEAD_CASES = [head_case((2, 12, 3, 16, 64), 1)]            # streaming 1x1 forward and (dW | dx) pass
for _shape in [(1, 38, 3, 72, 128), (2, 20, 3, 64, 68)]:     # head3.hip; swapped-role weight gradient through bnerv_tanh_grad, and the direct form
    for _flag in ("1", "0"):
        HEAD_CASES.append(head_case(_shape, 3, env={"BNERV_HEAD_SWAP": _flag}, tag=f" swap{_flag}"))


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: c.key.replace(" ", "_"))
def test_head_tanh(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- HNeRV up-conv
def upconv_case(shape):
    B, Cin, Cout, H, W, k, s, act = shape

    def make():
        g = torch.Generator().manual_seed(1000 * Cin + Cout)
        x = torch.randn(B, Cin, H, W, generator=g).requires_grad_(True)
        w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).requires_grad_(True)
        b = (torch.randn(Cout, generator=g) * 0.2).requires_grad_(True)
        return [x, w, b], torch.randn(B, Cout // (s * s), H * s, W * s, generator=g)
    return Case(f"upconv_act {_sid(shape)}", make, lambda x, w, b: _ref_upconv(x, w, b, s, act),
                lambda ops, x, w, b: ops.upconv_act(x, w, b, s, act), ["x", "w", "b"])


UPCONV_SHAPES = [(1, 39, 39, 30, 64, 5, 1, "gelu"), (1, 12, 48, 8, 32, 5, 2, "none"), (2, 33, 64, 17, 40, 5, 2, "gelu"),   # 5x5 kernels
                 (1, 80, 268, 45, 80, 3, 2, "gelu"), (1, 16, 96, 9, 16, 1, 1, "gelu")]                                   # bnerv_gelu_fwd / bnerv_mul vec gates


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", [upconv_case(s) for s in UPCONV_SHAPES], ids=lambda c: c.key.replace(" ", "_"))
def test_upconv_act(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- ConvNeXt block pieces
def dwconv_case(shape):
    B, Cc, H, W, K = shape

    def make():
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(B, Cc, H, W, generator=g).requires_grad_(True)
        w = (torch.randn(Cc, 1, K, K, generator=g) / K).requires_grad_(True)
        b = torch.randn(Cc, generator=g).requires_grad_(True)
        return [x, w, b], torch.randn(B, Cc, H, W, generator=g)
    return Case(f"dwconv {_sid(shape)}", make, lambda x, w, b: F.conv2d(x, w, b, padding=K // 2, groups=Cc),
                lambda ops, x, w, b: ops.dwconv(x, w, b), ["x", "w", "b"], exact=True)      # y and dx are the operator's own (aligned) tensors; nothing else is gated


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", [dwconv_case(s) for s in [(1, 64, 36, 64, 7), (1, 3, 9, 16, 3)]], ids=lambda c: c.key.replace(" ", "_"))
def test_dwconv(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


def _ln_ref(x, w, b):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + 1e-6)) + b[:, None, None]


def ln_case(shape):
    B, Cc, H, W = shape

    def make():
        g = torch.Generator().manual_seed(11)
        x = (torch.randn(B, Cc, H, W, generator=g) * 2 + 0.5).requires_grad_(True)
        w = (torch.rand(Cc, generator=g) + 0.5).requires_grad_(True)
        b = torch.randn(Cc, generator=g).requires_grad_(True)
        return [x, w, b], torch.randn(B, Cc, H, W, generator=g)
    return Case(f"layernorm_cf {_sid(shape)}", make, _ln_ref, lambda ops, x, w, b: ops.layernorm_cf(x, w, b, 1e-6), ["x", "w", "b"], exact=True)   # lnorm.hip: scalar for every operand


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("case", [ln_case(s) for s in [(1, 64, 36, 64), (3, 16, 9, 16)]], ids=lambda c: c.key.replace(" ", "_"))
def test_layernorm_cf(ops, case, variant, monkeypatch):
    run_variant(case, ops, *variant, monkeypatch)


def _cnx_ref(x, inp, w1, b1, w2, b2, gamma):
    h = F.gelu(F.conv2d(x, w1[:, :, None, None], b1))
    return inp + gamma[None, :, None, None] * F.conv2d(h, w2[:, :, None, None], b2)


CNX_NAMES = ["x", "inp", "w1", "b1", "w2", "b2", "gamma"]


def cnx_case(Cc, exact):
    def make():
        g = torch.Generator().manual_seed(100 + Cc)
        mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).requires_grad_(True)
        leaves = [mk(2, Cc, 18, 32), mk(2, Cc, 18, 32), mk(4 * Cc, Cc, sc=1 / math.sqrt(Cc)), mk(4 * Cc, sc=0.2), mk(Cc, 4 * Cc, sc=0.5 / math.sqrt(Cc)),
                  mk(Cc, sc=0.2), (torch.rand(Cc, generator=g) + 0.5).requires_grad_(True)]
        return leaves, torch.randn(2, Cc, 18, 32, generator=g)
    return Case(f"cnx_mlp C{Cc}", make, _cnx_ref, lambda ops, *gl: ops.cnx_mlp(*gl), CNX_NAMES, exact=exact)


# shifting a parameter: w1 / w2 are handed to the kernels as aligned copies, b1 / b2 / gamma are read element by element (b1 in 16-byte units
# only when aligned), and no other kernel's choice depends on them -> the aligned call's bits.  Shifting x / inp / the cotangent moves the k = 1 weight gradients to another kernel (wgrad1.hip needs aligned x, g).
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("which", ["w1", "w2", "b1", "b2", "gamma"])
@pytest.mark.parametrize("Cc", [16, 64])
def test_cnx_mlp_parameter_shifted(ops, Cc, which, k, monkeypatch):
    run_variant(cnx_case(Cc, True), ops, which, k, monkeypatch)


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("Cc", [16, 64])
def test_cnx_mlp(ops, Cc, variant, monkeypatch):
    run_variant(cnx_case(Cc, False), ops, *variant, monkeypatch)


def sft_case(shape):
    B, Cc, H, W = shape

    def make():
        g = torch.Generator().manual_seed(5)
        x = torch.randn(B, Cc, H, W, generator=g).requires_grad_(True)
        sc = torch.randn(B, Cc, 1, 1, generator=g).requires_grad_(True)
        sh = torch.randn(B, Cc, 1, 1, generator=g).requires_grad_(True)
        return [x, sc, sh], torch.randn(B, Cc, H, W, generator=g)
    return Case(f"sft_affine {_sid(shape)}", make, cpu_ref.sft_affine, lambda ops, x, sc, sh: ops.sft_affine(x, sc, sh), ["x", "scale", "shift"], exact=True)    # scalar for every operand


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
def test_sft_affine(ops, variant, monkeypatch):
    run_variant(sft_case((2, 12, 20, 36)), ops, *variant, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- dense layers
DENSE_SPECS = [(160, 256, "sin"), (160, 64, "sin"), (32, 32, "relu"), (32, 12, "none"), (256, 1152, "sin"), (32, 95, "none")]


def _dense_inputs(B):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(B, i, generator=g).requires_grad_(True) for i, _, _ in DENSE_SPECS]
    ws = [(torch.randn(o, i, 1, 1, generator=g) / math.sqrt(i)).requires_grad_(True) for i, o, _ in DENSE_SPECS]
    bs = [torch.randn(o, generator=g).requires_grad_(True) for _, o, _ in DENSE_SPECS]
    cots = [torch.randn(B, o, generator=g) for _, o, _ in DENSE_SPECS]
    return xs, ws, bs, cots


def _dense_run(ops, fn, xs, ws, bs, cots, idx_x, idx_p, shift_cot, k):
    """The six layers with the chosen operand groups shifted; returns outputs + gradients (xs, ws, bs order)."""
    keep = []

    def place(t, sh):
        v = gpu(t) if t.requires_grad else t.to(DEV)
        if sh:
            v, buf = shifted(v, k)
            check_shifted(v, k)
            keep.append((v, buf))
        return v
    xg, wg, bg = [place(t, idx_x) for t in xs], [place(t, idx_p) for t in ws], [place(t, idx_p) for t in bs]
    cg = [place(c, shift_cot) for c in cots]
    acts = [a for _, _, a in DENSE_SPECS]
    out = fn(xg, wg, bg, acts)
    seen = []
    for o in out:
        o.register_hook(lambda g_: seen.append(g_.data_ptr()))
    gg = torch.autograd.grad(out, xg + wg + bg, cg)
    assert sorted(seen) == sorted(c.data_ptr() for c in cg)
    for v, buf in keep:
        assert pads_intact(buf, k)
    return [o.detach() for o in out] + [g_.detach() for g_ in gg]


_DENSE_BASE = {}


def _dense_check(ops, route, B, which, k):
    fn = ops.dense_grouped if route == "grouped" else (lambda xs, ws, bs, acts: [ops.dense_gemm(x, w, b, a) for x, w, b, a in zip(xs, ws, bs, acts)])
    xs, ws, bs, cots = _dense_inputs(B)
    if (route, B) not in _DENSE_BASE:
        ld = [t.detach().double().requires_grad_(True) for t in xs + ws + bs]
        n = len(xs)
        ref = [cpu_ref._act(F.linear(x, w.flatten(1), b), a) for x, w, b, (_, _, a) in zip(ld[:n], ld[n:2 * n], ld[2 * n:], DENSE_SPECS)]
        rg = torch.autograd.grad(ref, ld, [c.double() for c in cots])
        runs = [_dense_run(ops, fn, xs, ws, bs, cots, False, False, False, k) for _ in range(2)]
        det = all(same(x, y) for x, y in zip(*runs))
        print(f"dense {route} B={B}: the aligned call gives the same bits twice: {det}")
        _DENSE_BASE[(route, B)] = ([r.detach().float() for r in ref] + [g_.float() for g_ in rg], runs[0], det)
    refs, base, det = _DENSE_BASE[(route, B)]
    got = _dense_run(ops, fn, xs, ws, bs, cots, which in ("x", "all"), which == "all", which in ("cot", "all"), k)
    n = len(DENSE_SPECS)
    for i, (a, r, b) in enumerate(zip(got, refs, base)):
        msg = f"dense {'fwd' if i < n else 'grad'} {i} [{route} B={B} {which} +{4 * k}B]"
        close(a, r, msg=msg + " vs float64")
        if det:     # the grouped kernels and the dense GEMM are scalar for every operand: the aligned call's bits
            assert same(a, b), msg + f": differs from the aligned call, max {float((a - b).abs().max()):.3e}"
        else:       # (the aligned call itself is not reproducible call to call: the operator's own tolerance)
            close(a, b, msg=msg + " vs aligned")


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("B", [1, 144])                     # 144: the MFMA GEMM route
def test_dense_grouped(ops, B, variant):
    _dense_check(ops, "grouped", B, *variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
def test_dense_gemm(ops, variant):
    _dense_check(ops, "gemm", 144, *variant)


# ---------------------------------------------------------------------------------------------------------------- time branch
@pytest.mark.parametrize("k", [1, 2])
def test_time_branch_declines_an_unaligned_weight_and_the_grouped_launches_take_it(ops, k):
    """widths (96, 128, 12) of test_time_branch_with_modulations_wider_than_one_dx_chunk with one modulation MLP weight shifted:
    ops.time_branch stages the weights with 16-byte loads and must decline (None); the caller's five-launch form -- PE, the two stem
    layers and the two modulation layers as grouped dense launches (model_blocks.mlp_pair_forward / tat_modulations) -- on the same
    shifted tensors must equal float64, outputs and every parameter gradient."""
    widths = (96, 128, 12)
    g = torch.Generator().manual_seed(11 + len(widths))
    Lv, SH, SO, TH, TO, B = 80, 256, 30 * 9 * 16, 64, 32, 1
    rn = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc)
    bases = (1.25 ** torch.arange(8, dtype=torch.float32).repeat_interleave(10)) * math.pi
    pos = torch.tensor([0.37], dtype=torch.float64)
    stem = [rn(SH, 2 * Lv, 1, 1, sc=0.08), rn(SH, sc=0.1), rn(SO, SH, 1, 1, sc=0.06), rn(SO, sc=0.1)]
    stem_t = [rn(TH, 2 * Lv, 1, 1, sc=0.08), rn(TH, sc=0.1), rn(TO, TH, 1, 1, sc=0.12), rn(TO, sc=0.1)]
    mlps = [[rn(TO, TO, 1, 1, sc=0.2), rn(TO, sc=0.1), rn(C_, TO, 1, 1, sc=0.2), rn(C_, sc=0.1)] for C_ in widths]
    flat = stem + stem_t + [t for m in mlps for t in m]
    cots = [rn(B, SO), rn(B, TO)] + [rn(B, C_) for C_ in widths]
    ps = [t.double().requires_grad_(True) for t in flat]
    arg = pos.float()[:, None] * bases[None, :]
    pe = torch.cat([torch.sin(arg), torch.cos(arg)], 1).double()
    lin = lambda x, w, b: x @ w.flatten(1).T + b
    so = torch.sin(lin(torch.sin(lin(pe, ps[0], ps[1])), ps[2], ps[3]))
    zt = torch.sin(lin(torch.sin(lin(pe, ps[4], ps[5])), ps[6], ps[7]))
    outs = [lin(torch.relu(lin(zt, ps[8 + 4 * i], ps[9 + 4 * i])), ps[10 + 4 * i], ps[11 + 4 * i]) for i in range(len(widths))]
    r_out = [so, zt] + outs
    r_g = torch.autograd.grad(r_out, ps, [c.double() for c in cots])

    pg = [t.to(DEV).requires_grad_(True) for t in flat]
    pd, bd = pos.to(DEV), bases.to(DEV)
    args = lambda p: (pd, bd, tuple(p[:4]), tuple(p[4:8]), [tuple(p[8 + 4 * i:12 + 4 * i]) for i in range(len(widths))])
    assert ops.time_branch(*args(pg)) is not None, "aligned: these shapes are the kernel's"
    keep = []
    for j in (4, 6, 10, 12):                                # stem_t's two layers, layer 1 of the first modulation MLP, layer 0 of the second
        one = list(pg)                                      # ONE weight shifted, every other tensor as allocated
        one[j], buf = shifted(pg[j], k)
        check_shifted(one[j], k)
        assert ops.time_branch(*args(one)) is None, f"weight {j} alone at +{4 * k} bytes must send the caller to the grouped launches"
    for j in (10, 12):                                      # the five-launch form below runs with two of them shifted
        pg[j], buf = shifted(pg[j], k)
        keep.append(buf)
    assert ops.time_branch(*args(pg)) is None
    pe_g = ops.positional_encoding(pd[:, None], bd, round_to_f32=True).view(B, -1)
    h0 = ops.dense_grouped([pe_g, pe_g], [pg[0], pg[4]], [pg[1], pg[5]], ["sin", "sin"])
    h1 = ops.dense_grouped(h0, [pg[2], pg[6]], [pg[3], pg[7]], ["sin", "sin"])
    n = len(widths)
    f0 = ops.dense_grouped([h1[1]] * n, [pg[8 + 4 * i] for i in range(n)], [pg[9 + 4 * i] for i in range(n)], ["relu"] * n)
    f1 = ops.dense_grouped(f0, [pg[10 + 4 * i] for i in range(n)], [pg[11 + 4 * i] for i in range(n)], ["none"] * n)
    got = [h1[0], h1[1]] + list(f1)
    for a, b in zip(got, r_out):
        close(a, b.float(), rtol=1e-4, atol=3e-5, msg="five-launch time branch fwd")
    gg = torch.autograd.grad(got, pg, [c.to(DEV) for c in cots])
    for i, (a, b) in enumerate(zip(gg, r_g)):
        close(a, b.float(), msg=f"five-launch time branch grad {i}")
    assert all(pads_intact(buf, k) for buf in keep)


# ---------------------------------------------------------------------------------------------------------------- loss / metrics
LOSS_TYPES = ["L1", "L2", "L1_freq", "Fusion10", "Fusion10_freq", "Fusion6", "L1_ssim_freq"]
_LOSS_BASE = {}


def _loss_all(ops, pg, td, lt):
    loss, stats = ops.loss_with_stats(pg, td, lt)
    grad, = torch.autograd.grad(loss, [pg])
    l2, st2, g2 = ops.loss_value_grad_stats(pg, td, lt)
    res = {"loss": loss.detach().reshape(1), "stats": stats, "grad": grad, "loss2": l2.reshape(1), "stats2": st2, "grad2": g2, "psnr": ops.psnr(pg, td)}
    if lt.startswith("Fusion10"):
        res["msssim"] = ops.msssim(pg, td)
    if lt in ("Fusion6", "L1_ssim_freq"):
        res["ssim"] = ops.ssim(pg, td)
    return {n: v.detach().clone() for n, v in res.items()}


# (2, 3, 176, 208): sides even down to level 3 -> the fused pyramid launch (loss.hip pyramid_body); (2, 3, 180, 270): the level-by-level means
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("which", ["pred", "target", "both"])
@pytest.mark.parametrize("lt", LOSS_TYPES)
@pytest.mark.parametrize("shape", [(2, 3, 176, 208), (2, 3, 180, 270)], ids=_sid)
def test_losses_and_metrics(ops, shape, lt, which, k):
    """loss_with_stats, loss_value_grad_stats, psnr, msssim, ssim.  No kernel of the loss path looks at the alignment of pred / target,
    so every result must carry the aligned call's bits."""
    key = (shape, lt)
    if key not in _LOSS_BASE:
        g = torch.Generator().manual_seed(sum(shape))
        tgt = torch.rand(*shape, generator=g)
        pred = (tgt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
        p64 = pred.double().requires_grad_(True)
        ref = loss_f64(p64, tgt.double(), lt) if lt in ("Fusion6", "L1_ssim_freq") else cpu_ref.loss_fn(p64, tgt.double(), lt)
        rgrad, = torch.autograd.grad(ref, [p64])
        refs = {"loss": ref.detach(), "grad": rgrad, "psnr": cpu_ref.psnr_fn_single(pred.double(), tgt.double())}
        if lt.startswith("Fusion10"):
            refs["msssim"] = msssim_ref.ms_ssim(pred.double(), tgt.double(), data_range=1, size_average=False)
        if lt in ("Fusion6", "L1_ssim_freq"):
            refs["ssim"] = msssim_ref.ssim(pred.double(), tgt.double(), data_range=1, size_average=False)
        runs = [_loss_all(ops, pred.to(DEV).requires_grad_(True), tgt.to(DEV), lt) for _ in range(2)]
        _LOSS_BASE[key] = (pred, tgt, refs, runs[0], all(same(runs[0][n], runs[1][n]) for n in runs[0]))
        print(f"{lt} {_sid(shape)}: the aligned call gives the same bits twice: {_LOSS_BASE[key][4]}")
    pred, tgt, refs, base, det = _LOSS_BASE[key]
    pg, td, keep = pred.to(DEV), tgt.to(DEV), []
    if which in ("pred", "both"):
        pg, buf = shifted(pg, k)
        check_shifted(pg, k)
        keep.append(buf)
    if which in ("target", "both"):
        td, buf = shifted(td, k)
        check_shifted(td, k)
        keep.append(buf)
    got = _loss_all(ops, pg.requires_grad_(True), td, lt)
    for name in ("loss", "loss2"):
        assert abs(got[name].item() - refs["loss"].item()) <= 2e-4 * abs(refs["loss"].item()), (name, got[name].item(), refs["loss"].item())
    for name in ("grad", "grad2"):
        close(got[name], refs["grad"], rtol=2e-3, atol=2e-3 * float(refs["grad"].abs().max()), msg=f"{lt} {name}")
    close(got["psnr"], refs["psnr"], rtol=1e-5, atol=1e-3, msg="psnr")
    close(got["stats"][:, 4], refs["psnr"], rtol=1e-5, atol=1e-3, msg="stats psnr")
    for name in ("msssim", "ssim"):
        if name in got:
            close(got[name], refs[name], rtol=1e-4, atol=1e-5, msg=name)
    for name, v in got.items():
        if det:
            assert same(v, base[name]), f"{lt} {_sid(shape)} [{which} +{4 * k}B] {name}: differs from the aligned call"
        else:       # (the aligned call itself is not reproducible: the value / gradient tolerances of the loss tests)
            close(v, base[name], rtol=2e-3, atol=2e-3 * float(base[name].abs().max()), msg=f"{lt} {name} vs aligned")
    assert all(pads_intact(buf, k) for buf in keep)


# ---------------------------------------------------------------------------------------------------------------- PE, CEM, optimizers
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_positional_encoding(ops, dtype):
    """pos shifted by one element (f32: +4 bytes, f64: +8), then bases shifted too: the aligned call's bits, and float64 sin / cos of the
    reference's product (fp32 product for fp32 positions, model_blocks.py:122; fp64 product for fp64 positions) within the 2e-6 of
    test_pe_against_reference_golden."""
    bases = (1.25 ** torch.arange(8, dtype=torch.float32).repeat_interleave(10)) * math.pi
    pos = torch.tensor([[0.37], [0.0], [0.91]], dtype=dtype)
    arg = (pos * bases[None, :]).double() if dtype == torch.float32 else pos * bases[None, :].double()
    ref = torch.cat([torch.sin(arg), torch.cos(arg)], 1)
    base = ops.positional_encoding(pos.to(DEV), bases.to(DEV))
    assert same(base, ops.positional_encoding(pos.to(DEV), bases.to(DEV)))
    ps, pbuf = shifted(pos.to(DEV), 1)
    check_shifted(ps, 1)
    bs, bbuf = shifted(bases.to(DEV), 1)
    check_shifted(bs, 1)
    for p_, b_ in ((ps, bases.to(DEV)), (pos.to(DEV), bs), (ps, bs)):
        got = ops.positional_encoding(p_, b_)
        assert float((got.view(3, -1).double().cpu() - ref).abs().max()) < 2e-6
        assert same(got, base)
    assert pads_intact(pbuf, 1) and pads_intact(bbuf, 1)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("training", [True, False])
def test_cem_scale_rate(ops, training, k):
    """The inputs of test_cem_fused_quantise_rate_vs_oracle with every weight tensor and scale shifted: against the oracle with that
    test's tolerances, and the aligned call's bits (the fused CEM kernels are scalar for every operand)."""
    from oracle import cem_ref
    g = torch.Generator().manual_seed(21)
    shapes = [(24, 12, 3, 3), (24,), (750, 30, 3, 3), (3,), (64, 160, 1, 1), (16,)]
    ws = [(torch.randn(*s, generator=g) * (0.05 if i != 5 else 1e-2) + (0.0 if i != 5 else 0.3)).requires_grad_(True) for i, s in enumerate(shapes)]
    scales = [cem_ref.scale_init(w.detach(), 8, True).reshape(1).clone().requires_grad_(True) for w in ws]
    scales[5] = torch.tensor([0.2], requires_grad=True)
    noises = [torch.rand(w.shape, generator=g) - 0.5 for w in ws]
    cots = [torch.randn(w.shape, generator=g) for w in ws]
    a = torch.tensor([1.0, 0.5, 2.0, -1.0, 0.25, 1.5])
    ref_bits, ref_deq = [], []
    for w, s, z in zip(ws, scales, noises):
        code, quant, deq = cem_ref.scale_t(w, s)
        ref_bits.append(cem_ref.cal_bitrate(code, quant, training, noise=z)["bitrate"])
        ref_deq.append(deq)
    ref_loss = sum(ai * b for ai, b in zip(a, ref_bits)) + sum((d * c).sum() for d, c in zip(ref_deq, cots))
    ref_g = torch.autograd.grad(ref_loss, ws + scales)

    def run(shift):
        keep = []

        def place(t):
            v = gpu(t)
            if shift:
                v, buf = shifted(v, k)
                check_shifted(v, k)
                keep.append(buf)
            return v
        wg, sg = [place(w) for w in ws], [place(s) for s in scales]
        bits, stats, deq = ops.cem_scale_rate(wg, sg, [z.to(DEV) for z in noises] if training else [None] * len(ws), training)
        loss = (bits * a.to(DEV)).sum() + sum((d * c.to(DEV)).sum() for d, c in zip(deq, cots))
        got = torch.autograd.grad(loss, wg + sg)
        assert all(pads_intact(buf, k) for buf in keep)
        return [bits.detach(), stats.detach()] + [d.detach() for d in deq] + [x.detach() for x in got]
    b0, b1, got = run(False), run(False), run(True)
    n = len(ws)
    for i in range(n):
        assert abs(got[0][i].item() - ref_bits[i].item()) <= 2e-4 * abs(ref_bits[i].item()) + 1e-2, (i, got[0][i].item(), ref_bits[i].item())
        torch.testing.assert_close(got[2 + i].cpu(), ref_deq[i].detach(), rtol=0, atol=0)
    for i, (x, r) in enumerate(zip(got[2 + n:], ref_g)):
        close(x, r, rtol=2e-3, atol=2e-3 * float(r.abs().max()) + 1e-6, msg=f"cem grad {i}")
    det = all(same(x, y) for x, y in zip(b0, b1))
    print(f"cem training={training}: the aligned call gives the same bits twice: {det}")
    for i, (x, y) in enumerate(zip(got, b0)):
        if det:
            assert same(x, y), f"cem result {i}: differs from the aligned call"
        else:       # (the aligned call is not reproducible call to call: the oracle tolerance of the gradients)
            close(x, y, rtol=2e-3, atol=2e-3 * float(y.abs().max()) + 1e-6, msg=f"cem result {i} vs aligned")


@pytest.mark.parametrize("name", ["Adan", "Adam"])
def test_fused_optimizers(name):
    """Three tensors of 5, 1025 and 70 000 elements, parameters and p.grad at +4 / +8 / +12 bytes, three steps: the same optimizer on
    aligned copies, bit for bit (the descriptor-table kernels of csrc/optim.hip are scalar per element), guard elements untouched."""
    from boosting_nerv_amd import optimizer
    g = torch.Generator().manual_seed(5)
    sizes = (5, 1025, 70000)
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * 0.1 for n in sizes] for _ in range(3)]
    pa = [t.to(DEV).requires_grad_(True) for t in p0]
    ps, pbufs, gs, gbufs = [], [], [], []
    for i, t in enumerate(p0):
        v, buf = shifted(t.to(DEV).requires_grad_(True), i + 1)
        check_shifted(v, i + 1)
        gv, gbuf = shifted(torch.zeros_like(t).to(DEV), 3 - i)
        check_shifted(gv, 3 - i)
        ps.append(v); pbufs.append(buf); gs.append(gv); gbufs.append(gbuf)
    oa, os_ = getattr(optimizer, name)(pa, lr=0.003), getattr(optimizer, name)(ps, lr=0.003)
    for step in range(3):
        for i in range(3):
            pa[i].grad = grads[step][i].to(DEV)
            gs[i].copy_(grads[step][i])
            ps[i].grad = gs[i]
            assert ps[i].grad.data_ptr() == gs[i].data_ptr()
        oa.step()
        os_.step()
        for i in range(3):
            assert torch.equal(ps[i].detach(), pa[i].detach()), (name, step, i)
            assert not torch.equal(pa[i].detach().cpu(), p0[i]), "the step changed nothing"
    for i in range(3):
        assert pads_intact(pbufs[i], i + 1) and pads_intact(gbufs[i], 3 - i)


# ----------------------------------------------------------------------------------------------------------------------
# raw wrappers: outputs, residuals and workspaces that a C-ABI caller owns
# ----------------------------------------------------------------------------------------------------------------------
RAW_LAYERS = [(12, 64, 128), (38, 24, 64)]                  # (channels, H, W): the conv4 family / the wide split kernels when aligned


def _raw_inputs(Cc, H, W):
    g = torch.Generator().manual_seed(Cc + H)
    x = torch.randn(1, Cc, H, W, generator=g)
    w = torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc)
    b = torch.randn(Cc, generator=g)
    sc, sh = torch.randn(1, Cc, generator=g) * 0.3, torch.randn(1, Cc, generator=g) * 0.3
    a0 = torch.randn(1, Cc, H, W, generator=g)
    gy = torch.randn(1, Cc, H, W, generator=g)
    return x, w, b, sc, sh, a0, gy


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("which", ["out", "aux0", "x"])
@pytest.mark.parametrize("layer", RAW_LAYERS, ids=_sid)
def test_raw_conv_with_caller_owned_buffers(ops, layer, which, k):
    """ops._conv (bnerv_conv_igemm) with the OUTPUT, the residual operand of EP_BIAS_RES, or the input at +4 k bytes: float64
    F.conv2d, and the NaN guards on both sides of a shifted output survive -- a vector store at a misaligned base must not spill."""
    from boosting_nerv_amd import _lib as L
    Cc, H, W = layer
    x, w, b, sc, sh, a0, _ = _raw_inputs(Cc, H, W)
    res = which == "aux0"
    xin = (x * (1 + sc[:, :, None, None]) + sh[:, :, None, None]) if res else x
    ref = F.conv2d(xin.double(), w.double(), b.double(), padding=1) + (a0.double() if res else 0)
    xd, a0d = x.to(DEV), a0.to(DEV)
    out, obuf = torch.full((1, Cc, H, W), NAN, device=DEV), None
    if which == "out":
        out, obuf = shifted(out, k)
        check_shifted(out, k)
    elif which == "aux0":
        a0d, abuf = shifted(a0d, k)
        check_shifted(a0d, k)
    else:
        xd, xbuf = shifted(xd, k)
        check_shifted(xd, k)
    kw = dict(B=1, Cin=Cc, Cout=Cc, H=H, W=W, k=3)
    if res:
        ops._conv(xd, w.to(DEV), b.to(DEV), out, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_RES, scale=sc.to(DEV), shift=sh.to(DEV), aux0=a0d, **kw)
    else:
        ops._conv(xd, w.to(DEV), b.to(DEV), out, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS, **kw)
    close(out, ref.float(), msg=f"raw conv fwd [{which} +{4 * k}B]")
    if obuf is not None:
        assert pads_intact(obuf, k), "the kernel wrote outside a shifted output"


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("which", ["dw", "g", "x"])
@pytest.mark.parametrize("layer", RAW_LAYERS, ids=_sid)
def test_raw_wgrad_with_caller_owned_buffers(ops, layer, which, k):
    """ops._wgrad (bnerv_conv_wgrad) with dw (and db), the gradient, or the input shifted: the float64 contraction, guards intact."""
    from boosting_nerv_amd import _lib as L
    Cc, H, W = layer
    x, w, _, _, _, _, gy = _raw_inputs(Cc, H, W)
    wr = w.double().requires_grad_(True)
    rw, = torch.autograd.grad(F.conv2d(x.double(), wr, None, padding=1), [wr], gy.double())
    rb = gy.double().sum((0, 2, 3))
    xd, gd = x.to(DEV), gy.to(DEV)
    dw, db = torch.full((Cc, Cc, 3, 3), NAN, device=DEV), torch.full((Cc,), NAN, device=DEV)
    bufs = []
    if which == "dw":
        dw, wbuf = shifted(dw, k)
        db, bbuf = shifted(db, k)
        check_shifted(dw, k)
        check_shifted(db, k)
        bufs = [wbuf, bbuf]
    elif which == "g":
        gd, gbuf = shifted(gd, k)
        check_shifted(gd, k)
    else:
        xd, xbuf = shifted(xd, k)
        check_shifted(xd, k)
    ops._wgrad(xd, gd, dw, db, B=1, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE)
    close(dw, rw.float(), msg=f"raw wgrad dw [{which} +{4 * k}B]")
    close(db, rb.float(), msg=f"raw wgrad db [{which} +{4 * k}B]")
    assert all(pads_intact(buf, k) for buf in bufs)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("layer", [(30, 9, 16), (12, 64, 128), (38, 24, 64)], ids=_sid)
def test_partial_buffer_sized_by_the_library_fits_the_kernel_that_runs(ops, layer, k):
    """One EP_DGELU_SAVED launch (the TAT block's conv1 data gradient) with the incoming gradient at +4 k bytes (k = 0: aligned).  The
    [rows, B, 2, Cout] partial buffer is sized from bnerv_conv_partial_rows for THAT descriptor -- 4x16 tiles for the low-resolution family,
    8x32 tiles for everything else, and alignment decides which runs (conv.hip bnerv_conv_partial_rows) -- and over-allocated by one
    NaN row: every row the library asked for is written, the extra row stays NaN, and output and reduced sums match float64.  (The
    descriptor is built by ops._conv_desc, as ops._conv builds it; _conv allocates the buffer itself, so the guarded call is made here.)  Then the same
    launch through ops._conv, whose own buffer must be sized from the descriptor it launches with: output and reduced sums again."""
    from boosting_nerv_amd import _lib as L
    Cc, H, W = layer
    lib = L.load()
    _, w, _, sc, _, a0, gy = _raw_inputs(Cc, H, W)
    g = torch.Generator().manual_seed(77)
    gp, h = torch.rand(1, Cc, H, W, generator=g), torch.randn(1, Cc, H, W, generator=g)
    v = F.conv_transpose2d(gy.double(), w.double(), padding=1)                     # d / d(input) of conv(., w)
    ref_out = v * (1 + sc.double()[:, :, None, None]) * gp.double()
    ref_sum = torch.stack([(v * h.double()).sum((2, 3)), v.sum((2, 3))], 1)         # [B, 2, C]: (ds, dt)
    gd, wd, gpd, hd, scd = gy.to(DEV), w.to(DEV), gp.to(DEV), h.to(DEV), sc.to(DEV)
    if k:
        gd, gbuf = shifted(gd, k)
        check_shifted(gd, k)
    out = torch.full((1, Cc, H, W), NAN, device=DEV)
    d = ops._conv_desc(gd, wd, None, out, B=1, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_PLAIN, ep_mode=L.EP_DGELU_SAVED, transposed=1,
                       aux0=gpd, aux1=hd, scale=scd)
    rows = lib.bnerv_conv_partial_rows(C.byref(d))
    small = Cc == 30 and k == 0                                                    # the low-resolution family takes 30 -> 30 at 9x16 only when aligned
    assert rows == (((H + 3) // 4) * ((W + 15) // 16) if small else lib.bnerv_conv_tiles(H, W))
    part = torch.full((rows + 1, 1, 2, Cc), NAN, device=DEV)
    d.partial = part.data_ptr()
    assert lib.bnerv_conv_partial_rows(C.byref(d)) == rows                         # the answer does not depend on `partial`
    L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(d)), "bnerv_conv_igemm")
    torch.cuda.synchronize()
    assert torch.isnan(part[rows]).all(), "the kernel wrote past the rows the library asked for"
    assert torch.isfinite(part[:rows]).all(), "a row the library asked for was never written"
    close(out, ref_out.float(), msg=f"dgelu-saved out [+{4 * k}B]")
    close(part[:rows].double().sum(0), ref_sum.float(), msg=f"dgelu-saved sums [+{4 * k}B]")
    # the same launch through ops._conv, which asks for the row count, allocates the buffer and reduces it itself: it must ask with the
    # descriptor (and so the pointers) it launches with
    _poison = [torch.full((n_, 1, 2, Cc), NAN, device=DEV) for n_ in (2, 3, rows) for _ in range(4)]
    del _poison                                              # free blocks of the candidate sizes hold NaN: a row never written shows
    out2 = torch.full((1, Cc, H, W), NAN, device=DEV)
    st = ops._conv(gd, wd, None, out2, B=1, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_PLAIN, ep_mode=L.EP_DGELU_SAVED, transposed=1,
                   aux0=gpd, aux1=hd, scale=scd)
    assert torch.isfinite(st).all(), "ops._conv reduced a partial row its kernel never wrote"
    close(out2, ref_out.float(), msg=f"dgelu-saved out through ops._conv [+{4 * k}B]")
    close(st, ref_sum.float(), msg=f"dgelu-saved sums through ops._conv [+{4 * k}B]")


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 64, 36, 64, 7), (1, 3, 9, 16, 3)], ids=_sid)
def test_raw_dwconv_with_a_shifted_output(ops, shape, k, flip):
    """bnerv_dwconv_fwd with y at +4 k bytes (forward, and the flipped-tap data-gradient form): float64, guards intact."""
    from boosting_nerv_amd import _lib as L
    B, Cc, H, W, K = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Cc, H, W, generator=g)
    w = torch.randn(Cc, 1, K, K, generator=g) / K
    b = torch.randn(Cc, generator=g)
    ref = F.conv2d(x.double(), (w.flip(2, 3) if flip else w).double(), None if flip else b.double(), padding=K // 2, groups=Cc)
    y, ybuf = shifted(torch.full((B, Cc, H, W), NAN, device=DEV), k)
    check_shifted(y, k)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    L.check(L.load().bnerv_dwconv_fwd(L.stream(), L.ptr(xd), L.ptr(wd), None if flip else L.ptr(bd), L.ptr(y), B, Cc, H, W, K, flip), "bnerv_dwconv_fwd")
    close(y, ref.float(), msg=f"raw dwconv fwd [y +{4 * k}B flip {flip}]")
    assert pads_intact(ybuf, k), "the kernel wrote outside a shifted output"


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("hw", [64 * 68, 9 * 16, 8192 + 4], ids=lambda v: f"HW{v}")
def test_raw_tanh_grad_with_shifted_operands(ops, hw, k):
    """bnerv_tanh_grad with HW % 4 == 0 and g, img or gt at +4 k bytes takes the scalar form (it used to refuse): float64 values and
    channel sums, guards of a shifted gt intact."""
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    B, Cc = 2, 3
    gen = torch.Generator().manual_seed(hw)
    g, img = torch.randn(B, Cc, hw, generator=gen), torch.rand(B, Cc, hw, generator=gen)
    ref = g.double() * 0.5 * (1 - (2 * img.double() - 1) ** 2)
    nblk = lib.bnerv_tanh_grad_blocks(hw)
    for which in ("g", "img", "gt"):
        gd, imd, gt = g.to(DEV), img.to(DEV), torch.full((B, Cc, hw), NAN, device=DEV)
        buf = None
        if which == "g":
            gd, _b = shifted(gd, k)
            check_shifted(gd, k)
        elif which == "img":
            imd, _b = shifted(imd, k)
            check_shifted(imd, k)
        else:
            gt, buf = shifted(gt, k)
            check_shifted(gt, k)
        part = torch.full((B * nblk, Cc), NAN, device=DEV)
        L.check(lib.bnerv_tanh_grad(L.stream(), L.ptr(gd), L.ptr(imd), L.ptr(gt), L.ptr(part), B, Cc, hw), "bnerv_tanh_grad")
        close(gt, ref.float(), msg=f"tanh_grad fwd [{which} +{4 * k}B]")
        close(part.double().sum(0), ref.sum((0, 2)).float(), msg=f"tanh_grad sums [{which} +{4 * k}B]")
        assert buf is None or pads_intact(buf, k)
