"""GPU tests (``-m gpu``) of the ConvNeXt encoder kernels at every instantiation and tile edge: ops.cnx_mlp, ops.dwconv,
ops.layernorm_cf, ops.dense_gemm and model_blocks.patchify_conv on every row of tests/encoder_cases.py, forward and all gradients against
the float64 references there -- element-wise results inside their running error bounds, sums over pixels inside close() of
test_gpu_ops.py -- and a set of bit-for-bit invariances (a pixel's result does not depend on where its tile sits in the launch).
Each test prints its largest err / bound before it asserts (``-s`` shows them)."""
import pytest
import torch

import encoder_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
cid = lambda c: c.id


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


def _leaf(t):
    return None if t is None else t.to(DEV).requires_grad_(True)


def _judge(op, name, check, got, ref):
    """Print the figures, then assert: no NaN, every bounded result within its bound, every summed result within close()."""
    for k, v in got.items():
        assert v is None or bool(torch.isfinite(v).all()), f"{op} {name}: {k} is not finite"
    ratios, oks = check({k: (None if v is None else v.detach().cpu()) for k, v in got.items()}, ref)
    for k, r in ratios.items():
        print(f"[encoder-ratio] {op}.{k} {name} {r:.4f}")
    assert all(r <= 1.0 for r in ratios.values()), (op, name, ratios)
    assert all(oks.values()), (op, name, oks)


# ------------------------------------------------------------------------------------------------------------ cnx_mlp
def run_cnx(ops, d):
    """ops.cnx_mlp and its backward under d['cot'] on the device -> the names encoder_cases.check_cnx reads (device tensors)."""
    leaves = {k: _leaf(d[k]) for k in E.CNX_LEAVES}
    out = ops.cnx_mlp(*(leaves[k] for k in E.CNX_LEAVES))
    names = [k for k in E.CNX_LEAVES if leaves[k] is not None]
    g = dict(zip(names, torch.autograd.grad(out, [leaves[k] for k in names], d["cot"].to(DEV))))
    return dict(out=out.detach(), dx=g["x"], dinp=g["inp"], dw1=g["w1"], db1=g["b1"], dw2=g["w2"], db2=g["b2"], dgamma=g.get("gamma"))


@pytest.mark.parametrize("c", E.CNX_CASES, ids=cid)
def test_cnx_mlp_case(ops, c):
    nt, grid, items = E.mlp_plan(c.B, c.C, c.H * c.W)
    assert nt == c.nt and (grid * 4 < items) == c.trip, (c, nt, grid, items)
    d = E.cnx_inputs(c)
    _judge("cnx_mlp", c.id, E.check_cnx, run_cnx(ops, d), E.cnx_reference(d))


def _cnx_row(C, B, H, W):
    return next(c for c in E.CNX_CASES if (c.C, c.B, c.H, c.W) == (C, B, H, W) and c.gamma and c.w1s == 1.0)


@pytest.mark.parametrize("B,H,W", [(2, 11, 757), (1, 257, 256)])
@pytest.mark.parametrize("C", [16, 64])
def test_cnx_mlp_pixels_do_not_depend_on_their_place_in_the_launch(ops, C, B, H, W):
    """out and dx of the first 4000 pixels of sample 0 and of the last 37 pixels of the last sample, each run as a call of its own
    (one tile per wave, first trip), bit for bit the same pixels of the large call (two tiles per wave; 257 x 256: second trip)."""
    HW = H * W
    c = E.Cnx(f"prefix-C{C}-{B}x{H}x{W}", B, C, H, W, 2, HW == 257 * 256, True, 1.0, "")
    nt, grid, items = E.mlp_plan(B, C, HW)
    assert nt == 2 and (grid * 4 < items) == c.trip
    d = E.cnx_inputs(c)
    big = run_cnx(ops, d)
    for b, lo, hi in ((0, 0, 4000), (B - 1, HW - 37, HW)):
        n = hi - lo
        assert E.mlp_plan(1, C, n)[0] == 1 and E.mlp_plan(1, C, n)[1] * 4 >= E.mlp_plan(1, C, n)[2]
        sub = dict(d, **{k: d[k].flatten(2)[b:b + 1, :, lo:hi].reshape(1, C, 1, n).contiguous() for k in ("x", "inp", "cot")})
        small = run_cnx(ops, sub)
        for k in ("out", "dx"):
            want = big[k].flatten(2)[b, :, lo:hi]
            assert torch.equal(small[k].reshape(C, n), want), (k, b, lo, float((small[k].reshape(C, n) - want).abs().max()))


@pytest.mark.parametrize("C", E.CNX_DIMS)
def test_cnx_mlp_forward_without_saved_activations_is_the_training_forward(ops, C):
    c = _cnx_row(C, 2, 11, 757)
    assert E.mlp_plan(c.B, C, c.H * c.W)[0] == 2
    d = E.cnx_inputs(c)
    args = [d[k].to(DEV) for k in E.CNX_LEAVES]
    with torch.no_grad():
        plain = ops.cnx_mlp(*args)
    train = ops.cnx_mlp(args[0].clone().requires_grad_(True), *args[1:])
    assert train.requires_grad and not plain.requires_grad
    assert torch.equal(plain, train.detach())


# ------------------------------------------------------------------------------------------------------------ dwconv
def run_dw(ops, d):
    x, w, b = (_leaf(d[k]) for k in ("x", "w", "b"))
    y = ops.dwconv(x, w, b)
    dx, dw, db = torch.autograd.grad(y, [x, w, b], d["cot"].to(DEV))
    return dict(y=y.detach(), dx=dx, dw=dw, db=db)


@pytest.mark.parametrize("c", E.DW_CASES, ids=cid)
def test_dwconv_case(ops, c):
    if c.groups is not None:
        assert E.dw_plan(c.B, c.C, c.H, c.W) == (c.groups, c.rows)
    d = E.dw_inputs(c)
    _judge("dwconv", c.id, E.check_dw, run_dw(ops, d), E.dw_reference(d))


@pytest.mark.parametrize("shape", [(1, 3, 17, 65, 7), (1, 2, 15, 68, 3)])
def test_dwconv_does_not_depend_on_where_the_image_sits(ops, shape):
    """y and dx of an image, bit for bit the crop of the same image placed at (5, 9) in a zero canvas 16 rows and 64 columns larger:
    taps on zeros add exact zeros, so the pixels at the seams and borders of one layout are interior pixels of the other."""
    c = next(c for c in E.DW_CASES if (c.B, c.C, c.H, c.W, c.K) == shape)
    d = E.dw_inputs(c)
    oy, ox = 5, 9

    def canvas(t):
        z = torch.zeros(c.B, c.C, c.H + 16, c.W + 64)
        z[:, :, oy:oy + c.H, ox:ox + c.W] = t
        return z
    small = run_dw(ops, d)
    large = run_dw(ops, dict(d, x=canvas(d["x"]), cot=canvas(d["cot"])))
    for k in ("y", "dx"):
        crop = large[k][:, :, oy:oy + c.H, ox:ox + c.W]
        assert torch.equal(small[k], crop), (k, float((small[k] - crop).abs().max()))


# ------------------------------------------------------------------------------------------------------------ layernorm_cf
def run_ln(ops, d):
    x, w, b = (_leaf(d[k]) for k in ("x", "w", "b"))
    y = ops.layernorm_cf(x, w, b, E.LN_EPS)
    dx, dw, db = torch.autograd.grad(y, [x, w, b], d["cot"].to(DEV))
    return dict(y=y.detach(), dx=dx, dw=dw, db=db)


@pytest.mark.parametrize("c", E.LN_CASES, ids=cid)
def test_layernorm_cf_case(ops, c):
    d = E.ln_inputs(c)
    _judge("layernorm_cf", c.id, E.check_ln, run_ln(ops, d), E.ln_reference(d))


@pytest.mark.parametrize("C", [7, 63])
def test_layernorm_cf_samples_do_not_depend_on_the_batch(ops, C):
    c = next(c for c in E.LN_CASES if (c.B, c.C, c.HW) == (3, C, 65))
    d = E.ln_inputs(c)
    whole = run_ln(ops, d)
    for b in range(c.B):
        one = run_ln(ops, dict(d, x=d["x"][b:b + 1].contiguous(), cot=d["cot"][b:b + 1].contiguous()))
        for k in ("y", "dx"):
            assert torch.equal(one[k][0], whole[k][b]), (k, b, float((one[k][0] - whole[k][b]).abs().max()))


# ------------------------------------------------------------------------------------------------------------ patchify / dense_gemm
@pytest.mark.parametrize("c", E.PATCH_CASES, ids=cid)
def test_patchify_conv_case(ops, c):
    from boosting_nerv_amd import model_blocks
    d = E.patch_inputs(c)
    conv = torch.nn.Conv2d(c.Cin, c.Cout, c.s, stride=c.s)
    with torch.no_grad():
        conv.weight.copy_(d["w"])
        conv.bias.copy_(d["b"])
    conv = conv.to(DEV)
    x = _leaf(d["x"])
    y = model_blocks.patchify_conv(x, conv)
    assert y.shape == d["cot"].shape
    dx, dw, db = torch.autograd.grad(y, [x, conv.weight, conv.bias], d["cot"].to(DEV))
    Hc, Wc = (c.H // c.s) * c.s, (c.W // c.s) * c.s
    assert Hc < c.H and Wc < c.W or "cropped" not in c.hits
    assert not bool(dx[:, :, Hc:].any()) and not bool(dx[:, :, :, Wc:].any()), "input gradient on the rows / columns the stride crops away"
    _judge("patchify", c.id, E.check_patch, dict(y=y.detach(), dx=dx, dw=dw, db=db), E.patch_reference(d))


@pytest.mark.parametrize("rows,I,O", E.GEMM_CASES)
def test_dense_gemm_at_the_row_split_threshold(ops, rows, I, O):
    d = E.gemm_inputs(rows, I, O)
    x, w, b = (_leaf(d[k]) for k in ("x", "w", "b"))
    y = ops.dense_gemm(x, w, b)
    dx, dw, db = torch.autograd.grad(y, [x, w, b], d["cot"].to(DEV))
    _judge("dense_gemm", f"{rows}x{I}x{O}", E.check_patch, dict(y=y.detach(), dx=dx, dw=dw, db=db), E.gemm_reference(d))
