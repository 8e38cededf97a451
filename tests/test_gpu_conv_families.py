"""GPU tests (``-m gpu``) of every shipped conv kernel instantiation, family asserted: the cases of tests/conv_family_cases.py, launched
through the C ABI on descriptors built by ops._conv_desc / ops._wgrad_desc, against the float64 reference of tests/conv_desc_ref.py.

Exact pass: small dyadic operands (tests/test_conv_family_cases_cpu.py proves that equality is owed on them).  Every linear result --
out, (ds, dt), dw, db -- must EQUAL the float64 result; zero tolerance, `==` so that -0.0 passes.  A single missing or duplicated
product is a plain inequality, whatever K is.  Behind a non-linear epilogue or prologue the pre-activation is still exact and only the
function's own error is allowed: sin / cos 3e-7, gelu 3e-7 (1 + |u|), gelu' 6e-7 (test_sincos_epilogue_accuracy,
test_gelu_pair_epilogue_accuracy); tanh has no bound of its own in the project and takes the forward tolerance of close().

Random pass: seeded normal operands, a distinct scale per (b, c); |kernel - float64| <= BOUND * sum |a| |b| per element.  For the
split-bf16 kernels BOUND is the stated contract 3.5e-7 (tools/split_contract.py).  For the f32-MFMA families no contract was ever
written down, and none is invented here: the bound is the worst case of ANY f32 chain of K_eff terms, (K_eff + 2) 2^-24 -- a property
of f32, not of the kernels.  It is LOOSE (observed ratios are a few percent of it: DESIGN.md, "f32 contract per family"); it catches a
precision downgrade and errors that small dyadic values mask, such as a wrong scale index.  The exact pass is the sharp check.
What exactly is allowed -- bias and residual folded into the sum as tools/split_contract.py folds them, the slope and function bounds, and
the one rounding term (the tanh-grad prologue) -- is spelled out in conv_family_cases.conv_allowance / wgrad_allowance; the weight
gradients' db is held to the same coefficient times sum |g|.

The IN_GELU_AFFINE cases are NOT sharp in the exact pass: gelu(x) is not dyadic, so the contraction behind it rounds like any other, and
these cases get the random pass's allowance there too (the gelu bound carried through |W| plus the chain bound)."""
import ctypes as C

import pytest
import torch

import conv_desc_ref as R
import conv_family_cases as K
from boosting_nerv_amd import _lib as L
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = K.build()
NAN = float("nan")
GUARD = 64          # floats behind an EP_PLAIN workspace that must stay NaN


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


def _env(monkeypatch, env):
    for k in K.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _dev(t):
    return {n: v.to(DEV).contiguous() for n, v in t.items()}


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _equal(tag, got, ref64):
    got, ref = got.detach().cpu(), ref64.float()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    bad = (got != ref).nonzero()
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{tag}: {len(bad)}/{ref.numel()} elements differ from float64; first at {i}: kernel {got[i].item()!r}, float64 {ref[i].item()!r}, "
                             f"difference {got[i].item() - ref[i].item()!r}")


def _within(tag, got, ref64, allow, fam=None, scale=None):
    """|got - float64| <= allow per element; prints the worst ratio to the allowance and, given scale = sum |a| |b|, the worst error in units
    of it: the figure an f32 contract of the family would be written in ("f32 contract per family")."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{tag}: not finite"
    err = (got - ref64).abs()
    ratio = (err / allow.clamp_min(1e-300)).max().item()
    print(f"RATIO {fam or '-'} {tag}: worst |err| / allowance = {ratio:.3g}, worst |err| = {err.max().item():.3e}")
    if scale is not None:
        print(f"CONTRACT {fam or '-'} {tag}: worst |err| / sum|a||b| = {(err / scale.clamp_min(1e-300)).max().item():.3g}")
    bad = err > allow
    assert not bad.any(), f"{tag}: {int(bad.sum())}/{err.numel()} beyond the allowance, worst ratio {ratio:.3f}"


def _conv_buffers(c):
    so = K._conv_shapes(c)[3]
    return _nan(*so), (_nan(*so) if c.get("out2") else None)


def _launch_conv(ops, c, t, d_t, fam_check=True, launch=True):
    """Descriptor on real tensors, `partial` sized by the library plus a NaN guard, family asserted, one bnerv_conv_igemm / bnerv_conv5_igemm."""
    lib = L.load()
    out, out2 = _conv_buffers(c)
    kw = {n: d_t.get(n) for n in ("aux0", "aux1", "aux2", "scale", "shift")}
    d = ops._conv_desc(d_t["x"], d_t["w"], d_t.get("bias"), out, B=c["B"], Cin=c["Cin"], Cout=c["Cout"], H=c["H"], W=c["W"], k=c["k"], in_mode=c["in_mode"],
                       ep_mode=c["ep_mode"], in_s=c["in_s"], out_s=c["out_s"], transposed=c["transposed"], out2=out2,
                       **({"ctx": None} if (c["kind"] == "conv5" or not c.get("ctx", True)) else {}), **kw)
    part = rows = ws = None
    if c["kind"] == "conv5":
        nbytes = lib.bnerv_conv5_ws_bytes(c["Cin"], c["Cout"])
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        if launch:
            L.check(lib.bnerv_conv5_igemm(L.stream(), C.byref(d), L.ptr(ws), nbytes), "bnerv_conv5_igemm")
        return dict(d=d, out=out, out2=out2, part=None, rows=None, ws=ws, keep=(d_t, ws))
    if c["ep_mode"] in R.SUMS_EP:
        rows = lib.bnerv_conv_partial_rows(C.byref(d))
        part = _nan(rows + 1, c["B"], 2, c["Cout"])
        d.partial = part.data_ptr()
    elif c["ep_mode"] == L.EP_PLAIN and c["partial"]:
        nbytes = lib.bnerv_conv_splitk_ws_bytes(C.byref(d))
        assert nbytes > 0 and nbytes % 4 == 0, (K.case_id(c), nbytes)
        ws = _nan(nbytes // 4 + GUARD)
        d.partial = ws.data_ptr()
        rows = nbytes // 4
    if fam_check:
        fam = lib.bnerv_conv_family(C.byref(d), None)
        assert L.CONV_FAM[fam] == c["family"], f"{K.case_id(c)}: the real descriptor runs on {L.CONV_FAM[fam]}"
    if launch:
        L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(d)), "bnerv_conv_igemm")
    return dict(d=d, out=out, out2=out2, part=part, rows=rows, ws=ws, keep=(d_t,))


def _check_conv(ops, c, t, r, run, exact, split, fam):
    tag = K.case_id(c) + (" exact" if exact else " random")
    if run["ws"] is not None and c["kind"] == "conv":
        assert torch.isnan(run["ws"][run["rows"]:]).all(), f"{tag}: wrote past the workspace the library asked for"
    st = None
    if run["part"] is not None:
        rows, part = run["rows"], run["part"]
        assert torch.isnan(part[rows]).all(), f"{tag}: wrote past the rows the library asked for"
        assert torch.isfinite(part[:rows]).all(), f"{tag}: a row the library asked for was never written"
        st = torch.empty(c["B"], 2, c["Cout"], device=DEV)
        ops._reduce_slabs(part, rows, c["B"] * 2 * c["Cout"], st)
    torch.cuda.synchronize()
    assert torch.isfinite(run["out"]).all(), f"{tag}: out has elements that were never written"
    if exact and K.out_exact(c):
        _equal(tag + " out", run["out"], r["out"])
        if st is not None:
            _equal(tag + " (ds, dt)", st, r["sums"])
        return
    allow = K.conv_allowance(c, t, r, split, exact_pre=exact and K.pre_exact(c))
    if allow["out"] is None:                                # tanh head: the project's forward tolerance; the worst error is printed for a later bound
        err = (run["out"].cpu().double() - r["out"]).abs().max().item()
        print(f"TANH {tag}: worst |err| = {err:.3e}")
        close(run["out"], r["out"].float(), msg=tag + " fwd")
    else:
        scale = None
        if not exact and c["ep_mode"] in (L.EP_PLAIN, L.EP_BIAS):      # a linear epilogue: the error is the contraction's own
            scale = K.reference(c, t, absolute=True)["v"]
            scale = torch.nn.functional.pixel_shuffle(scale, c["out_s"]) if c["out_s"] > 1 else scale
        _within(tag + " out", run["out"], r["out"], allow["out"], fam=fam, scale=scale)
    if run["out2"] is not None:
        _within(tag + " out2", run["out2"], r["out2"], allow["out2"], fam=fam)
    if st is not None:
        if exact and K.pre_exact(c):                        # EP_DGELU: dt is linear in v
            _equal(tag + " dt", st[:, 1], r["sums"][:, 1])
        _within(tag + " (ds, dt)", st, r["sums"], allow["sums"], fam=fam)


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("case", CASES["conv"], ids=K.case_id)
def test_conv_family(ops, case, mode, monkeypatch):
    c, exact = case, mode == "exact"
    _env(monkeypatch, c["env"])
    t = K.conv_operands(c, exact)
    r = K.reference(c, t)
    run = _launch_conv(ops, c, t, _dev(t))
    ops._flush_deferred()
    _check_conv(ops, c, t, r, run, exact, split=c["family"] == "wide_bf16", fam="conv/" + c["family"])


def _launch_wgrad(ops, c, d_t, fam_check=True, launch=True, defer=False):
    lib = L.load()
    k = c["k"]
    dw, db = _nan(c["Cout"], c["Cin"], k, k), (_nan(c["Cout"]) if c["db"] else None)
    five = c["kind"] == "conv5_wgrad"
    nbytes = lib.bnerv_conv5_wgrad_ws_bytes(c["B"], c["Cin"], c["Cout"], c["H"], c["W"]) if five else lib.bnerv_conv_wgrad_ws_bytes(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], k)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    d = ops._wgrad_desc(d_t["x"], d_t["g"], dw, db, ws, nbytes, B=c["B"], Cin=c["Cin"], Cout=c["Cout"], H=c["H"], W=c["W"], k=k, in_mode=c["in_mode"], g_mode=c["g_mode"],
                        g_s=c["g_s"], gaux=d_t.get("gaux"), scale=d_t.get("scale"), shift=d_t.get("shift"), defer=defer, **({"ctx": None} if five else {}))
    if fam_check and not five:
        fam = lib.bnerv_conv_wgrad_family(C.byref(d), None)
        assert L.WGRAD_FAM[fam] == c["family"], f"{K.case_id(c)}: the real descriptor runs on {L.WGRAD_FAM[fam]}"
    if launch:
        L.check((lib.bnerv_conv5_wgrad if five else lib.bnerv_conv_wgrad)(L.stream(), C.byref(d)), "weight gradient")
    return dict(d=d, dw=dw, db=db, keep=(d_t, ws))


def _check_wgrad(c, t, r, run, exact, split, fam, tag=None):
    tag = (tag or K.case_id(c)) + (" exact" if exact else " random")
    torch.cuda.synchronize()
    names = ("dw", "db") if run["db"] is not None else ("dw",)
    for n in names:
        assert torch.isfinite(run[n]).all(), f"{tag}: {n} has elements that were never written"
    if exact and K.out_exact(c):
        for n in names:
            _equal(f"{tag} {n}", run[n], r[n])
        return
    allow = K.wgrad_allowance(c, t, split)
    ab = K.reference(c, t, absolute=True)
    for n in names:
        _within(f"{tag} {n}", run[n], r[n], allow[n], fam=fam, scale=ab[n])


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("case", CASES["wgrad"], ids=K.case_id)
def test_wgrad_family(ops, case, mode, monkeypatch):
    c, exact = case, mode == "exact"
    _env(monkeypatch, c["env"])
    t = K.wgrad_operands(c, exact)
    r = K.reference(c, t)
    run = _launch_wgrad(ops, c, _dev(t))
    ops._flush_deferred()
    _check_wgrad(c, t, r, run, exact, split=c["family"] in K.SPLIT_WGRAD, fam="wgrad/" + c["family"])


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("case", CASES["pair"], ids=K.case_id)
def test_pair_form(ops, case, mode, monkeypatch):
    """One bnerv_conv_wgrad_pair call on the descriptors ops._wgrad_conv_pair builds (shared gradient, the TAT epilogue's raw operand as the
    weight gradient's input): rc 0 on the named form, both halves held to the stand-alone assertions.  The conv half of the wide
    form is held to the split contract.  The weight half is held to the bound of the family that bnerv_conv_wgrad_family names for its real
    descriptor: the forms pair the stand-alone family's role, and beside the low-resolution conv (small_wide) that is always one of the two
    wide families, so 3.5e-7 there as well."""
    exact = mode == "exact"
    _env(monkeypatch, case["env"])
    lib = L.load()
    cv, tc, wg, tw = K.pair_operands(case, exact)
    rc_, rw_ = K.reference(cv, tc), K.reference(wg, tw)
    dc = _dev(tc)
    dwt = {n: (dc["x"] if v is tc["x"] else dc.get("aux0") if v is tc.get("aux0") else dc.get("aux1") if v is tc.get("aux1") else dc.get("scale") if v is tc.get("scale")
               else v.to(DEV).contiguous()) for n, v in tw.items()}
    crun = _launch_conv(ops, cv, tc, dc, fam_check=False, launch=False)
    wrun = _launch_wgrad(ops, wg, dwt, fam_check=False, launch=False, defer=True)
    rows = C.c_int(-1)
    form = lib.bnerv_conv_wgrad_pair_form(C.byref(crun["d"]), C.byref(wrun["d"]), C.byref(rows))
    assert (L.PAIR_FORM[form] if form >= 0 else "none") == case["form"], K.case_id(case)
    if crun["part"] is not None:
        assert rows.value == crun["rows"]
    assert lib.bnerv_conv_wgrad_pair(L.stream(), C.byref(crun["d"]), C.byref(wrun["d"])) == 0, lib.bnerv_last_error()
    ops._flush_deferred()
    wfam = L.WGRAD_FAM[lib.bnerv_conv_wgrad_family(C.byref(wrun["d"]), None)]
    if case["form"] in ("small_wide", "bf16_wide"):
        assert wfam in K.SPLIT_WGRAD, (K.case_id(case), wfam)
    _check_conv(ops, cv, tc, rc_, crun, exact, split=case["form"] == "bf16_wide", fam="pair/" + case["form"])
    _check_wgrad(wg, tw, rw_, wrun, exact, split=wfam in K.SPLIT_WGRAD, fam="pair/" + case["form"], tag=K.case_id(case) + " weight half")


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("case", CASES["conv5"], ids=K.case_id)
def test_conv5(ops, case, mode, monkeypatch):
    c, exact = case, mode == "exact"
    _env(monkeypatch, c["env"])
    if c["kind"] == "conv5":
        t = K.conv_operands(c, exact)
        r = K.reference(c, t)
        run = _launch_conv(ops, c, t, _dev(t))
        _check_conv(ops, c, t, r, run, exact, split=True, fam="conv5")
    else:
        t = K.wgrad_operands(c, exact)
        r = K.reference(c, t)
        run = _launch_wgrad(ops, c, _dev(t))
        _check_wgrad(c, t, r, run, exact, split=True, fam="conv5_wgrad")
