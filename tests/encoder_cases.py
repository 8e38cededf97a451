"""Float64 references, error bounds and case tables for the ConvNeXt encoder kernels of HNeRV_Boost: the fused MLP tail
(cnx_mlp_* in csrc/gemm.hip), the depthwise conv (csrc/dwconv.hip), the channels-first LayerNorm (csrc/lnorm.hip) and the patchify GEMM
(dense_gemm).  Plain CPU code on stock torch ops; tests/test_encoder_cases_cpu.py checks the tables and the bounds without a device,
tests/test_gpu_encoder_ops.py runs every row on the GPU.

Two kinds of check:

  element-wise results (a fixed, short chain of fp32 operations per element) are held to a RUNNING ERROR BOUND computed in float64 from
  the fp32 operands, u = 2^-24:
    cnx_mlp out   P = |W1||x| + |b1|, dpre = (C+1) u P;  dhid = 1.13 dpre + 3e-7 (1 + |pre|)  (1.13 >= |gelu'|; 3e-7 (1 + |v|) is what
                  test_gpu_ops.test_gelu_pair_epilogue_accuracy asserts for this GELU);  dY = |W2| dhid + (4C+1) u (|W2||hid| + |b2|);
                  dout = |gamma| dY + 2u (|inp| + |gamma Y|)
    cnx_mlp dx    the same through W2^T, gelu' and W1^T; gelu' carries 6e-7 (same test) + 1.0 * dpre (|gelu''| <= 0.80, and the backward
                  reads the fp32 pre-activations the forward saved)
    dwconv y, dx  (K*K+1) u (|w| * |x| + |b|)
    patchify / dense_gemm y, dx   (Kc+1) u (|a||b| + |bias|), Kc the contraction length
  sums over pixels (every parameter gradient) and the LayerNorm results use the suite's standing tolerance, close() of test_gpu_ops.py
  against float64.  Inputs are zero-mean random, so a lost 16-pixel tile moves such a sum by far more than that tolerance
  (test_encoder_cases_cpu.py shows it for every row).

Largest err / bound observed on an MI355X (for the record; the assertions use the bounds above, never these figures):
    cnx_mlp out   0.060  nt2-C16-2x27x309            cnx_mlp dx    0.046  nt2-C16-2x16x521
    dwconv y      0.72   1x1x33x130-k1               dwconv dx     0.48   1x1x33x130-k1
    patchify y    0.064  2x3x181x322-s5-o64          patchify dx   0.17   3x16x9x17-s2-o16
    dense_gemm y  0.34   513x7x5                     dense_gemm dx 0.37   512x7x5
  The dwconv figures are those of K = 1, where the bound has no slack to give: one product and one bias add are two roundings of up to
  u each against a bound of 2u (the ratio falls as K grows: at most 0.37 at K = 3, 0.11 at K = 7).  Every bit-for-bit invariance of test_gpu_encoder_ops.py held.
"""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
CNX_DIMS = (16, 32, 48, 64)
GELU_ERR, DGELU_ERR, DGELU_MAX, D2GELU_MAX = 3e-7, 6e-7, 1.13, 1.0


# ------------------------------------------------------------------------------------------------------------ plan queries
def mlp_plan(B, C, HW):
    """(nt, grid_blocks, items) of bnerv_cnx_mlp_plan: what the cnx_mlp launchers would launch for [B, C, HW]."""
    from boosting_nerv_amd import _lib as L
    nt, grid, items = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.load().bnerv_cnx_mlp_plan(B, C, HW, ctypes.byref(nt), ctypes.byref(grid), ctypes.byref(items))
    assert rc == 0, (rc, L.load().bnerv_last_error())
    return nt.value, grid.value, items.value


def dw_plan(B, C, H, W):
    """(groups, rows_per_group) of bnerv_dwconv_wgrad_plan."""
    from boosting_nerv_amd import _lib as L
    groups, rows = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.load().bnerv_dwconv_wgrad_plan(B, C, H, W, ctypes.byref(groups), ctypes.byref(rows))
    assert rc == 0, (rc, L.load().bnerv_last_error())
    return groups.value, rows.value


# ------------------------------------------------------------------------------------------------------------ case tables
# nt / trip: what the plan must say (trip: grid_blocks * 4 < items, the persistent loop runs a second time);  tail: HW % 32
Cnx = collections.namedtuple("Cnx", "id B C H W nt trip gamma w1s hits")


def _cnx_cases():
    rows = []

    def add(tag, B, C, H, W, nt, trip=False, gamma=True, w1s=1.0, hits=""):
        rows.append(Cnx(f"{tag}-C{C}-{B}x{H}x{W}", B, C, H, W, nt, trip, gamma, w1s, hits))
    for C in CNX_DIMS:
        add("hw5", 1, C, 1, 5, 1, hits="HW < 16: one partial tile")
    for C in CNX_DIMS:
        add("tail63", 3, C, 7, 9, 1, hits="B > 1, HW = 63: ragged tail of every sample at NT = 1")
    add("thr", 1, 16, 128, 128, 1, hits="16384 pixels: the last size at NT = 1")
    add("thr", 1, 16, 127, 131, 2, hits="16637 pixels: NT = 2")
    for H, W, what in ((16, 520, "HW % 32 = 0"), (11, 757, "HW % 32 = 7: second half-tile dead"),
                       (16, 521, "HW % 32 = 16: first half-tile exactly full"), (27, 309, "HW % 32 = 23: second half-tile partial")):
        for C in (CNX_DIMS if H * W == 8327 else (16, 64)):
            add("nt2", 2, C, H, W, 2, hits="NT = 2, B = 2, " + what)
    add("trip2", 1, 64, 150, 221, 2, trip=True, hits="NT = 2: 1036 items over 1024 wave slots")
    for C in (16, 32, 48):
        add("trip2", 1, C, 257, 256, 2, trip=True, hits="NT = 2: 2056 items over 2048 wave slots")
    add("trip1", 100, 64, 7, 23, 1, trip=True, hits="NT = 1: 1100 items over 1024 wave slots")
    add("nogamma", 3, 16, 7, 9, 1, gamma=False, hits="gamma None: backward without bnerv_cnx_param_grads")
    add("nogamma", 2, 64, 11, 757, 2, gamma=False, hits="gamma None at NT = 2")
    for C in CNX_DIMS:
        add("sat", 3, C, 7, 9, 1, w1s=30.0, hits="w1 x 30: pre-activations O(30), GELU saturates")
    return rows


CNX_CASES = _cnx_cases()

# groups / rows: what bnerv_dwconv_wgrad_plan must say (None: not what the row is there for)
Dw = collections.namedtuple("Dw", "id B C H W K groups rows hits")
DW_TILE_H, DW_TILE_W = 16, 64


def _dw(B, C, H, W, K, hits, groups=None, rows=None):
    return Dw(f"{B}x{C}x{H}x{W}-k{K}", B, C, H, W, K, groups, rows, hits)


DW_CASES = [
    _dw(1, 1, 1, 1, 7, "single pixel"),
    _dw(1, 2, 3, 3, 7, "image smaller than the kernel"),
    _dw(1, 1, 33, 130, 1, "K = 1"),
    _dw(1, 3, 17, 65, 7, "second tile column holds one column; scalar stores"),
    _dw(2, 2, 16, 67, 5, "three columns in the second tile column"),
    _dw(1, 2, 15, 68, 3, "vector stores across the seam"),
    _dw(8, 64, 80, 20, 7, "2 groups of 3 tile rows, the last holds 2", groups=2, rows=3),
    _dw(16, 64, 40, 20, 3, "one group holds all 3 tile rows", groups=1, rows=3),
]

Ln = collections.namedtuple("Ln", "id B C HW")
LN_C = (1, 2, 3, 4, 7, 17, 48, 63, 64)
LN_HW = (1, 63, 64, 65, 257)
LN_EPS = 1e-6
LN_CASES = [Ln(f"{B}x{C}x{HW}", B, C, HW) for B, C, HW in (
    (1, 1, 1), (3, 1, 65), (1, 2, 63), (3, 2, 257), (1, 3, 64), (3, 3, 1), (1, 4, 65), (3, 4, 63), (1, 7, 257), (3, 7, 65),
    (1, 17, 64), (3, 17, 63), (1, 48, 65), (3, 63, 65), (1, 63, 257), (1, 64, 63), (3, 64, 257))]

Patch = collections.namedtuple("Patch", "id B Cin H W s Cout split hits")
GEMM_SPLIT_ROWS = 512                        # bnerv_dense_gemm_bwd_ws_bytes is nonzero from this many rows on


def _patch(B, Cin, H, W, s, Cout, hits):
    rows = B * (H // s) * (W // s)
    return Patch(f"{B}x{Cin}x{H}x{W}-s{s}-o{Cout}", B, Cin, H, W, s, Cout, rows >= GEMM_SPLIT_ROWS, hits)


PATCH_CASES = [
    _patch(2, 3, 181, 322, 5, 64, "4608 rows: row-split weight gradient; both sides cropped"),
    _patch(1, 64, 37, 65, 3, 64, "252 rows: no split; K = 576; both sides cropped"),
    _patch(3, 16, 9, 17, 2, 16, "96 rows, K = 64"),
]
GEMM_CASES = [(511, 7, 5), (512, 7, 5), (513, 7, 5)]       # (rows, I, O): either side of the row-split threshold


# ------------------------------------------------------------------------------------------------------------ checks
def bound_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (float64); an element whose bound is 0 must be exact (else inf); nan -> inf."""
    got, ref, bound = got.detach().double().cpu(), ref.detach(), bound.detach()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def close_ok(got, ref, msg):
    """The suite's standing tolerance (close() of test_gpu_ops.py) as a predicate; nan fails."""
    from test_gpu_ops import close
    if bool(torch.isnan(got.detach()).any()):
        return False
    try:
        close(got, ref, msg=msg)
    except AssertionError:
        return False
    return True


def verdict(got, ref, bounded, summed, fwd=()):
    """{name: ratio} for the names in `bounded` (ref[name], ref['e_' + name]) and {name: bool} for those in `summed` (close());
    names in `fwd` use close()'s forward form.  Every name must be present in `got`."""
    ratios = {n: bound_ratio(got[n], ref[n], ref["e_" + n]) for n in bounded}
    oks = {n: close_ok(got[n], ref[n], msg=f"{n} fwd" if n in fwd else f"{n} grad") for n in summed}
    return ratios, oks


def passes(ratios, oks):
    return all(r <= 1.0 for r in ratios.values()) and all(oks.values())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ cnx_mlp
CNX_BOUNDED, CNX_SUMMED = ("out", "dx"), ("dw1", "db1", "dw2", "db2", "dgamma")
CNX_LEAVES = ("x", "inp", "w1", "b1", "w2", "b2", "gamma")


def cnx_inputs(c):
    """fp32 operands of a Cnx row (gamma None when the row says so) and the cotangent `cot`; seeded by the row."""
    g = _gen(1000 + 7 * c.C + c.B * c.H * c.W)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    C = c.C
    d = dict(x=rn(c.B, C, c.H, c.W), inp=rn(c.B, C, c.H, c.W), w1=rn(4 * C, C, sc=c.w1s / math.sqrt(C)), b1=rn(4 * C, sc=0.2),
             w2=rn(C, 4 * C, sc=0.5 / math.sqrt(C)), b2=rn(C, sc=0.2), gamma=torch.rand(C, generator=g) + 0.5, cot=rn(c.B, C, c.H, c.W))
    if not c.gamma:
        d["gamma"] = None
    return d


def cnx_ref(x, inp, w1, b1, w2, b2, gamma):
    """inp + gamma * pwconv2(gelu(pwconv1(x))) on stock ops, in the dtype of its operands (gamma may be None)."""
    y = F.conv2d(F.gelu(F.conv2d(x, w1[:, :, None, None], b1)), w2[:, :, None, None], b2)
    return inp + (y if gamma is None else gamma[None, :, None, None] * y)


def cnx_stock(d, dtype=torch.float32, drop_hidden=None, lose_tail=0):
    """Forward and every gradient by autograd over cnx_ref in `dtype` -> the names check_cnx reads.
    drop_hidden = j: hidden unit j does not reach pwconv2.  lose_tail = n: the last n pixels of the last sample are lost -- zero in
    out and dx, absent from every sum over pixels."""
    leaves = {k: d[k].to(dtype).clone().requires_grad_(True) for k in CNX_LEAVES if d[k] is not None}
    args = dict(leaves, gamma=leaves.get("gamma"))
    if drop_hidden is not None:
        keep = torch.ones(d["w2"].shape[1], dtype=dtype)
        keep[drop_hidden] = 0
        args["w2"] = leaves["w2"] * keep
    out = cnx_ref(*(args[k] for k in CNX_LEAVES))
    cot = d["cot"].to(dtype).clone()
    n = min(lose_tail, c_hw(d))
    if n:
        cot.flatten(2)[-1, :, -n:] = 0
    names = [k for k in CNX_LEAVES if k in leaves]
    grads = dict(zip(names, torch.autograd.grad(out, [leaves[k] for k in names], cot)))
    got = dict(out=out.detach().clone(), dx=grads["x"], dinp=grads["inp"], dw1=grads["w1"], db1=grads["b1"], dw2=grads["w2"], db2=grads["b2"],
               dgamma=grads.get("gamma"))
    if n:
        got["out"].flatten(2)[-1, :, -n:] = 0
    return got


def c_hw(d):
    return d["x"].shape[2] * d["x"].shape[3]


def cnx_reference(d):
    """Float64 results of cnx_mlp and of its backward under `cot`, written out (no autograd), with the running error bounds of the
    module docstring as e_out and e_dx.  Keys: out, dx, dinp, dw1, db1, dw2, db2, dgamma (None without gamma), e_out, e_dx."""
    B, C, H, W = d["x"].shape
    HW = H * W
    x, xin, cot = (d[k].double().reshape(B, C, HW) for k in ("x", "inp", "cot"))
    w1, b1, w2, b2 = (d[k].double() for k in ("w1", "b1", "w2", "b2"))
    gm = torch.ones(C, dtype=torch.float64) if d["gamma"] is None else d["gamma"].double()
    pre = w1 @ x + b1[:, None]                                                   # [B, 4C, HW]
    dpre = (C + 1) * U * (w1.abs() @ x.abs() + b1.abs()[:, None])
    cdf = 0.5 * (1 + torch.erf(pre / math.sqrt(2.0)))
    gd = cdf + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2 * math.pi)         # gelu'
    hid = pre * cdf
    del cdf
    dhid = DGELU_MAX * dpre + GELU_ERR * (1 + pre.abs())
    y = w2 @ hid + b2[:, None]
    dy = w2.abs() @ dhid + (4 * C + 1) * U * (w2.abs() @ hid.abs() + b2.abs()[:, None])
    del dhid, pre
    gy = gm[:, None] * y
    r = dict(out=xin + gy, e_out=gm.abs()[:, None] * dy + 2 * U * (xin.abs() + gy.abs()))
    del dy, gy
    # backward: dYv = gamma * cot; dG = W2^T dYv; dH = dG * gelu'; dX = W1^T dH
    dyv = gm[:, None] * cot
    e_dyv = U * dyv.abs() if d["gamma"] is not None else torch.zeros_like(dyv)
    dg = w2.t() @ dyv
    e_dg = w2.abs().t() @ e_dyv + (C + 1) * U * (w2.abs().t() @ dyv.abs())
    dh = dg * gd
    e_dh = gd.abs() * e_dg + dg.abs() * (DGELU_ERR + D2GELU_MAX * dpre) + U * dh.abs()
    del dg, e_dg, gd, dpre
    r["dx"] = w1.t() @ dh
    r["e_dx"] = w1.abs().t() @ e_dh + (4 * C + 1) * U * (w1.abs().t() @ dh.abs())
    del e_dh
    r["dinp"] = cot
    r["dw1"] = torch.einsum("bhp,bcp->hc", dh, x)
    r["db1"] = dh.sum((0, 2))
    S, t = torch.einsum("bcp,bhp->ch", cot, hid), cot.sum((0, 2))
    r["dw2"], r["db2"] = gm[:, None] * S, gm * t
    r["dgamma"] = (cot * y).sum((0, 2)) if d["gamma"] is not None else None
    for k in ("out", "e_out", "dx", "e_dx", "dinp"):
        r[k] = r[k].reshape(B, C, H, W)
    return r


def check_cnx(got, ref):
    """(ratios of out and dx against their bounds, close() verdicts of the parameter gradients); the gradient with respect to inp
    is the cotangent itself and must be exact."""
    summed = [n for n in CNX_SUMMED if ref[n] is not None]
    assert (ref["dgamma"] is None) == (got["dgamma"] is None)
    ratios, oks = verdict(got, ref, CNX_BOUNDED, summed)
    oks["dinp"] = bool(torch.equal(got["dinp"].detach().double().cpu(), ref["dinp"]))
    return ratios, oks


# ------------------------------------------------------------------------------------------------------------ dwconv
DW_BOUNDED, DW_SUMMED = ("y", "dx"), ("dw", "db")


def dw_inputs(c):
    g = _gen(2000 + c.B * 31 + c.C * 17 + c.H * 7 + c.W + c.K)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(x=rn(c.B, c.C, c.H, c.W), w=rn(c.C, 1, c.K, c.K, sc=1.0 / c.K), b=rn(c.C, sc=0.2), cot=rn(c.B, c.C, c.H, c.W))


def dwconv_ref(x, w, b):
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2, groups=x.shape[1])


def dw_last_tile_column(W):
    """First column of the last 64-wide tile column of a row of W pixels."""
    return ((W - 1) // DW_TILE_W) * DW_TILE_W


def _shift_last_tile_column(t):
    """Every pixel of the last tile column takes its left neighbour's value (0 at the left edge of the image)."""
    x0 = dw_last_tile_column(t.shape[-1])
    out = t.clone()
    out[..., x0:] = F.pad(t, (1, 0))[..., x0:t.shape[-1]]
    return out


def dw_stock(d, dtype=torch.float32, drop_tap=False, shift=False, lose_tile=False):
    """y and the gradients by autograd over dwconv_ref in `dtype`.  drop_tap: the centre tap of every channel is not applied (forward
    and data gradient).  shift: the last tile column of y and dx is shifted by one.  lose_tile: the last 16 x 64 tile of the last plane
    is absent from dw and db."""
    x, w, b = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b"))
    wf = w
    if drop_tap:
        keep = torch.ones(w.shape[-2:], dtype=dtype)
        keep[w.shape[-1] // 2, w.shape[-1] // 2] = 0
        wf = w * keep
    y = dwconv_ref(x, wf, b)
    cot = d["cot"].to(dtype).clone()
    if lose_tile:
        H, W = cot.shape[-2:]
        cot[-1, -1, ((H - 1) // DW_TILE_H) * DW_TILE_H:, dw_last_tile_column(W):] = 0
    dx, dw, db = torch.autograd.grad(y, [x, w, b], cot)
    y = y.detach()
    if shift:
        y, dx = _shift_last_tile_column(y), _shift_last_tile_column(dx)
    return dict(y=y, dx=dx, dw=dw, db=db)


def dw_reference(d):
    x, w, b, cot = (d[k].double() for k in ("x", "w", "b", "cot"))
    K = w.shape[-1]
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = dwconv_ref(xl, wl, bl)
    dx, dw, db = torch.autograd.grad(y, [xl, wl, bl], cot)
    e = (K * K + 1) * U
    return dict(y=y.detach(), dx=dx, dw=dw, db=db, e_y=e * dwconv_ref(x.abs(), w.abs(), b.abs()),
                e_dx=e * dwconv_ref(cot.abs(), w.abs().flip(-1, -2), None))


def check_dw(got, ref):
    return verdict(got, ref, DW_BOUNDED, DW_SUMMED)


# ------------------------------------------------------------------------------------------------------------ layernorm_cf
LN_SUMMED = ("y", "dx", "dw", "db")


def ln_inputs(c):
    g = _gen(3000 + c.B * 1009 + c.C * 17 + c.HW)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(x=rn(c.B, c.C, c.HW, 1), w=rn(c.C) * 0.5 + 1.0, b=rn(c.C, sc=0.2), cot=rn(c.B, c.C, c.HW, 1))


def lncf_ref(x, w, b, eps, leave_out=0):
    """w (x - u) / sqrt(s + eps) + b over dim 1, u = mean_c x, s = mean_c (x - u)^2.  leave_out = 1: the last channel is missing from
    the sum behind u (a mutation for the CPU test)."""
    C = x.shape[1]
    u = x[:, :C - leave_out].sum(1, keepdim=True) / C
    s = ((x - u) ** 2).mean(1, keepdim=True)
    return w[None, :, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[None, :, None, None]


def ln_stock(d, dtype=torch.float32, leave_out=0, lose_block=False):
    """lose_block: the last (partial) 64-pixel block of the last sample is absent from dw and db."""
    x, w, b = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b"))
    y = lncf_ref(x, w, b, LN_EPS, leave_out)
    cot = d["cot"].to(dtype).clone()
    if lose_block:
        HW = cot.shape[2]
        cot[-1, :, ((HW - 1) // 64) * 64:] = 0
    dx, dw, db = torch.autograd.grad(y, [x, w, b], cot)
    return dict(y=y.detach(), dx=dx, dw=dw, db=db)


def ln_reference(d):
    return ln_stock(d, torch.float64)


def check_ln(got, ref):
    return verdict(got, ref, (), LN_SUMMED, fwd=("y",))


# ------------------------------------------------------------------------------------------------------------ patchify / dense_gemm
PATCH_BOUNDED, PATCH_SUMMED = ("y", "dx"), ("dw", "db")


def patch_inputs(c):
    g = _gen(4000 + c.B + c.Cin * 3 + c.H * 5 + c.W * 7 + c.s)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    Ho, Wo = c.H // c.s, c.W // c.s
    return dict(x=rn(c.B, c.Cin, c.H, c.W), w=rn(c.Cout, c.Cin, c.s, c.s, sc=1.0 / math.sqrt(c.Cin * c.s * c.s)), b=rn(c.Cout, sc=0.2),
                cot=rn(c.B, c.Cout, Ho, Wo))


def patchify_ref(x, w, b):
    return F.conv2d(x, w, b, stride=w.shape[-1])


def gemm_inputs(rows, I, O):
    g = _gen(5000 + rows)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(x=rn(rows, I), w=rn(O, I, sc=1.0 / math.sqrt(I)), b=rn(O, sc=0.2), cot=rn(rows, O))


def _affine_stock(fn, d, dtype, drop_weight, lose_rows):
    x, w, b = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b"))
    wf = w
    if drop_weight:
        keep = torch.ones_like(w.detach())
        keep.flatten()[-1] = 0
        wf = w * keep
    y = fn(x, wf, b)
    cot = d["cot"].to(dtype).clone()
    if lose_rows:                                           # the last 16 GEMM rows (output pixels of the last sample) leave the sums
        if cot.dim() == 2:
            cot[-lose_rows:] = 0
        else:
            cot[-1].flatten(1)[:, -lose_rows:] = 0
    dx, dw, db = torch.autograd.grad(y, [x, w, b], cot)
    return dict(y=y.detach(), dx=dx, dw=dw, db=db)


def patch_stock(d, dtype=torch.float32, drop_weight=False, lose_rows=0):
    return _affine_stock(patchify_ref, d, dtype, drop_weight, lose_rows)


def gemm_stock(d, dtype=torch.float32, drop_weight=False, lose_rows=0):
    return _affine_stock(F.linear, d, dtype, drop_weight, lose_rows)


def patch_reference(d):
    """Float64 F.conv2d with stride = kernel size and its gradients; e_y with Kc = Cin s s, e_dx with Kc = Cout (0, so exact, on the
    rows and columns the stride crops away)."""
    r = patch_stock(d, torch.float64)
    x, w, b, cot = (d[k].double() for k in ("x", "w", "b", "cot"))
    s = w.shape[-1]
    r["e_y"] = (w[0].numel() + 1) * U * patchify_ref(x.abs(), w.abs(), b.abs())
    e_dx = F.conv_transpose2d(cot.abs(), w.abs(), None, stride=s)
    r["e_dx"] = (w.shape[0] + 1) * U * F.pad(e_dx, (0, x.shape[3] - e_dx.shape[3], 0, x.shape[2] - e_dx.shape[2]))
    return r


def gemm_reference(d):
    r = gemm_stock(d, torch.float64)
    x, w, b, cot = (d[k].double() for k in ("x", "w", "b", "cot"))
    r["e_y"] = (w.shape[1] + 1) * U * (x.abs() @ w.abs().t() + b.abs())
    r["e_dx"] = (w.shape[0] + 1) * U * (cot.abs() @ w.abs())
    return r


def check_patch(got, ref):
    return verdict(got, ref, PATCH_BOUNDED, PATCH_SUMMED)
