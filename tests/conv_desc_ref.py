"""Float64 reference of the conv descriptors of include/bnerv.h (bnerv_conv_desc, bnerv_wgrad_desc and their k = 5 forms), written
from the semantics tables of the header -- prologue, F.conv2d (or the flipped, swapped weight of `transposed`), epilogue, pixel shuffle --
in plain torch on the CPU.  `d` is a dict of the descriptor's integer fields, `t` a dict of tensors by the descriptor's pointer names
(any dtype; missing or None = NULL).  Every function returns float64 and, under "mid", every intermediate the header's formulas name,
so that a test can check them for exact representability.

absolute=True evaluates the same contraction on absolute values: sum |a| |b| per output element, the scale of the f32 contract
(tools/split_contract.py)."""
import math

import torch
import torch.nn.functional as F

IN_PLAIN, IN_AFFINE, IN_GELU_AFFINE, IN_UNSHUFFLE, IN_TANHGRAD = 0, 1, 2, 3, 4
EP_BIAS, EP_BIAS_SIN, EP_BIAS_RES, EP_BIAS_TANH, EP_PLAIN, EP_DGELU, EP_DSIN, EP_BIAS_GELU, EP_DGELU_SAVED = 0, 1, 2, 3, 4, 5, 6, 7, 8
SUMS_EP = (EP_DGELU, EP_DSIN, EP_DGELU_SAVED)


def gelu(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _f64(t, name):
    v = t.get(name)
    return None if v is None else v.detach().double().cpu()


def _bc(v):
    return v.reshape(v.shape[0], -1)[:, :, None, None]


def prologue(mode, s, x, scale=None, shift=None, aux=None, mul=None):
    """a = prologue(x) in conv space [B, Cin, H, W]; `mul` (k = 5 forms: aux0 / gaux, stored like x) multiplies x element-wise first."""
    if mul is not None:
        x = x * mul
    if mode == IN_PLAIN:
        return x
    if mode == IN_AFFINE:
        return x * (1 + _bc(scale)) + _bc(shift)
    if mode == IN_GELU_AFFINE:
        return gelu(x) * (1 + _bc(scale)) + _bc(shift)
    if mode == IN_UNSHUFFLE:                   # a[c*s*s + i*s + j][y][x] = x[c][y*s + i][x*s + j]
        return F.pixel_unshuffle(x, s) if s > 1 else x
    if mode == IN_TANHGRAD:
        return x * (0.5 * (1 - (2 * aux - 1) ** 2))
    raise ValueError(mode)


def effective_weight(d, w):
    """W(co, ci, t): w[co][ci][t] forward, w[ci][co][k*k-1-t] for the data gradient."""
    return w.transpose(0, 1).flip(2, 3).contiguous() if d.get("transposed", 0) else w


def conv_ref(d, t, v_delta=None, absolute=False, in_mul=None):
    """dict(out, out2, sums [B, 2, Cout] = (ds, dt), v, mid).  v_delta: added to the conv result v before the epilogue (a comparator's
    self-test removes one product with it).  absolute: only `v` = sum |a| |W| is meaningful (and returned as out)."""
    x, w = _f64(t, "x"), _f64(t, "w")
    in_mode, ep, k = d["in_mode"], d["ep_mode"], d["k"]
    in_s, out_s = d.get("in_s", 1), d.get("out_s", 1)
    scale, shift, bias = _f64(t, "scale"), _f64(t, "shift"), _f64(t, "bias")
    aux0, aux1, aux2 = _f64(t, "aux0"), _f64(t, "aux1"), _f64(t, "aux2")
    prologue_reads_scale = in_mode in (IN_AFFINE, IN_GELU_AFFINE)
    a = prologue(in_mode, in_s, x, scale if prologue_reads_scale else None, shift, aux0 if in_mode == IN_TANHGRAD else None,
                 None if in_mul is None else in_mul.double())
    assert a.shape == (d["B"], d["Cin"], d["H"], d["W"]), (a.shape, d)
    weff = effective_weight(d, w)
    assert weff.shape == (d["Cout"], d["Cin"], k, k), (weff.shape, d)
    if absolute:
        v = F.conv2d(a.abs(), weff.abs(), padding=(k - 1) // 2)
        return dict(out=v, v=v, a=a.abs(), weff=weff.abs())
    v = F.conv2d(a, weff, padding=(k - 1) // 2)
    if v_delta is not None:
        v = v + v_delta
    mid = dict(a=a, v=v)
    out2 = sums = None
    b = 0 if bias is None else bias[None, :, None, None]
    if ep == EP_PLAIN:
        out = v
    elif ep == EP_BIAS:
        out = v + b
    elif ep == EP_BIAS_SIN:
        mid["u"] = u = v + b
        out, out2 = torch.sin(u), torch.cos(u)
    elif ep == EP_BIAS_RES:
        mid["u"] = v + b
        out = v + b + aux0
    elif ep == EP_BIAS_TANH:
        mid["u"] = u = v + b
        out = torch.tanh(u) * 0.5 + 0.5
    elif ep == EP_BIAS_GELU:
        mid["u"] = u = v + b
        out, out2 = gelu(u), gelu_grad(u)
    elif ep in (EP_DGELU, EP_DGELU_SAVED):
        gp, gl = (gelu_grad(aux0), gelu(aux0)) if ep == EP_DGELU else (aux0, aux1)
        mid["vs"] = vs = v * (1 + _bc(scale))
        out = vs * gp
        mid["v_aux"] = va = v * gl
        sums = torch.stack([va.sum((2, 3)), v.sum((2, 3))], 1)
        mid["sum_abs"] = torch.stack([va.abs().sum((2, 3)), v.abs().sum((2, 3))], 1)
    elif ep == EP_DSIN:
        mid["vs"] = vs = v * (1 + _bc(scale))
        mid["t"] = tt = aux1 + vs
        out = tt if aux2 is None else tt * aux2
        mid["v_aux"] = va = v * aux0
        sums = torch.stack([va.sum((2, 3)), v.sum((2, 3))], 1)
        mid["sum_abs"] = torch.stack([va.abs().sum((2, 3)), v.abs().sum((2, 3))], 1)
    else:
        raise ValueError(ep)
    mid["out_conv_space"] = out
    if out_s > 1:
        out = F.pixel_shuffle(out, out_s)
        out2 = None if out2 is None else F.pixel_shuffle(out2, out_s)
    return dict(out=out, out2=out2, sums=sums, v=v, mid=mid, a=a, weff=weff)


def wgrad_ref(d, t, absolute=False, g_mul=None):
    """dict(dw [Cout, Cin, k, k], db [Cout], mid): dw[co][ci][t] = sum_{b,p} g[b][co][p] a[b][ci][p + t - pad], db[co] = sum_{b,p} g[b][co][p];
    a = prologue(x), g gathered by g_mode (PLAIN, UNSHUFFLE(g_s), TANHGRAD(gaux)); g_mul: the k = 5 form's gaux multiplier."""
    x, g = _f64(t, "x"), _f64(t, "g")
    k, g_mode = d["k"], d["g_mode"]
    a = prologue(d["in_mode"], 1, x, _f64(t, "scale"), _f64(t, "shift"))
    gc = prologue(g_mode, d.get("g_s", 1), g, aux=_f64(t, "gaux") if g_mode == IN_TANHGRAD else None, mul=None if g_mul is None else g_mul.double())
    assert a.shape == (d["B"], d["Cin"], d["H"], d["W"]) and gc.shape == (d["B"], d["Cout"], d["H"], d["W"]), (a.shape, gc.shape, d)
    if absolute:
        a, gc = a.abs(), gc.abs()
    cols = F.unfold(a, k, padding=(k - 1) // 2)                                     # [B, Cin*k*k, H*W]: a[b][ci][p + t - pad], zero outside
    dw = torch.einsum("bop,bkp->ok", gc.flatten(2), cols).reshape(d["Cout"], d["Cin"], k, k)
    db = gc.sum((0, 2, 3))
    return dict(dw=dw, db=db, mid=dict(a=a, g=gc), a=a, g=gc)


def conv5_ref(d, t, **kw):
    """bnerv_conv5_igemm: the k = 5 descriptor; a non-NULL aux0 multiplies the input element-wise before the gather."""
    assert d["k"] == 5 and d["in_mode"] in (IN_PLAIN, IN_UNSHUFFLE) and d["ep_mode"] in (EP_BIAS, EP_BIAS_GELU, EP_PLAIN)
    return conv_ref(d, {n: v for n, v in t.items() if n != "aux0"}, in_mul=t.get("aux0"), **kw)


def conv5_wgrad_ref(d, t, **kw):
    """bnerv_conv5_wgrad: in_mode PLAIN; a non-NULL gaux multiplies the stored gradient element-wise before the gather."""
    assert d["k"] == 5 and d["in_mode"] == IN_PLAIN and d["g_mode"] in (IN_PLAIN, IN_UNSHUFFLE)
    return wgrad_ref(d, {n: v for n, v in t.items() if n != "gaux"}, g_mul=t.get("gaux"), **kw)


def abs_bound(kind, d, t):
    """sum |a| |b| per output element: of v for the conv kinds, dict(dw, db) for the weight gradients."""
    if kind == "conv":
        return conv_ref(d, t, absolute=True)["v"]
    if kind == "conv5":
        return conv5_ref(d, t, absolute=True)["v"]
    r = wgrad_ref(d, t, absolute=True) if kind == "wgrad" else conv5_wgrad_ref(d, t, absolute=True)
    return dict(dw=r["dw"], db=r["db"])


def quantum(*tensors):
    """The largest power of two of which every element of every tensor is an integer multiple (1.0 for all-zero input)."""
    q = 1.0
    for t in tensors:
        t = t.double()
        while not bool((t / q == torch.round(t / q)).all()):
            q /= 2
            assert q > 2.0 ** -60, "not dyadic"
    return q
