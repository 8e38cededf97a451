"""GPU tests (``-m gpu``) of the mixed-radix LDS FFT behind the spectral loss term (csrc/fft_body.h, instantiated in csrc/loss.hip for
bnerv_loss_fwd_bwd -- generic radices 7..31 -- and for bnerv_loss_ssim_fwd_bwd -- 7..37) against the float64 reference of
tests/fft_loss_ref.py, at the sizes where the kernels take another path than at the 720p / 1080p frames of the train step:

  * two generic (prime >= 7) stages on an axis: the first of them multiplies by twiddles other than 1;
  * every generic radix 7..31 (and 37 in the single-scale SSIM path) as a first and as a last stage, on rows and on columns;
  * odd W (no kept column but 0 is its own mirror), an odd number of rows (a lone last row without a partner);
  * rows longer than 2048 (the tail loop of the table copy) and than 2560 (the multi-batch adjoint row pass); columns longer than 2048;
  * sides of 1 and 2 (no stage at all, one kept column);
  * the largest frame the LDS takes, and the refusal beyond it.

Asserted are the project's own tolerances (test_gpu_ops.test_loss_against_goldens_and_oracle): value 2e-4 relative, gradient rtol 2e-3
with atol 2e-3 max|ref|.  Every case PRINTS its real errors next to those of torch.fft.fft2 in float32 on the CPU (run with -s; the
worst figures per radix class are in DESIGN.md next to "Tolerances as tested").  A wrong sign or mirror weight moves every pixel of a
plane by up to 4 gscale against an atol of about 8e-3 sqrt(2 H W) gscale: caught while H W is below ~125 000, which most frames are."""
import ctypes as C

import pytest
import torch

import fft_loss_ref as R
from test_gpu_ops import close
from test_gpu_ssim_loss import loss_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAL_RTOL, GRAD_RTOL = 2e-4, 2e-3
ids = lambda s: "x".join(map(str, s))      # noqa: E731


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


_inputs = {}


def inputs(shape):
    """(pred, tgt, float64 per-sample value, float64 gradient of the batch mean) of a case: made once, shared, never written to."""
    if shape not in _inputs:
        pred, tgt, census = R.make_inputs(shape, R.case_seed(shape))
        assert census == 0, (shape, census)
        _inputs[shape] = (pred, tgt, R.spectral_loss_f64(pred, tgt), R.spectral_grad_f64(pred, tgt))
    return _inputs[shape]


FILL = -7.0


def spectral_call(pg, td, want_grad=True):
    """bnerv_loss_fwd_bwd with c_fft = 1 and nothing else, through the C ABI -> (return code, loss [1], stats [B, 5], grad or None).  The
    outputs start out filled with FILL."""
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    B, Cc, H, W = pg.shape
    nbytes = lib.bnerv_loss_ws_bytes(B, Cc, H, W, 0, 1)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), FILL, device=DEV)
    stats = torch.full((B, L.LOSS_STATS), FILL, device=DEV)
    grad = torch.full_like(pg, FILL) if want_grad else None
    d = L.LossDesc(L.ptr(pg), L.ptr(td), L.ptr(grad), L.ptr(loss), L.ptr(stats), L.ptr(ws), nbytes, B, Cc, H, W, 0.0, 0.0, 0.0, 1.0)
    rc = lib.bnerv_loss_fwd_bwd(L.stream(), C.byref(d))
    torch.cuda.synchronize()
    return rc, loss, stats, grad


def f32_cpu_errors(pred, tgt, ref_b, rgrad):
    """(relative value error, max|grad - ref| / max|ref|) of torch.fft.fft2 in float32 on the CPU: the yardstick of the report."""
    p = pred.clone().requires_grad_(True)
    v = torch.view_as_real(torch.fft.fft2(p) - torch.fft.fft2(tgt)).abs().flatten(1).mean(1).mean()
    g, = torch.autograd.grad(v, [p])
    ref = ref_b.mean().item()
    return abs(v.item() - ref) / ref, float((g.double() - rgrad).abs().max() / rgrad.abs().max())


def check_pure_spectral(ops, shape, label):
    from boosting_nerv_amd import _lib as L
    pred, tgt, ref_b, rgrad = inputs(shape)
    ops.prepare_loss(shape[2], shape[3])
    pg, td = pred.to(DEV), tgt.to(DEV)
    rc, loss, stats, grad = spectral_call(pg, td)
    L.check(rc, "bnerv_loss_fwd_bwd")
    ref = ref_b.mean().item()
    verr = abs(loss.item() - ref) / ref
    gerr = float((grad.cpu().double() - rgrad).abs().max() / rgrad.abs().max())
    cv, cg = f32_cpu_errors(pred, tgt, ref_b, rgrad)
    flag = "  ** above 8x the float32 CPU figure **" if verr > 8 * cv or gerr > 8 * cg else ""
    print(f"\n[fft-error] {label} {ids(shape):>14} {R.radix_class(shape):>12}: value rel err {verr:.2e} (f32 CPU {cv:.2e}), "
          f"max|grad - ref| / max|ref| {gerr:.2e} (f32 CPU {cg:.2e}){flag}")
    assert verr <= VAL_RTOL, (loss.item(), ref)
    sb = stats[:, 0].cpu().double()
    assert float(((sb - ref_b).abs() / ref_b).max()) <= VAL_RTOL, (sb, ref_b)
    close(grad, rgrad, rtol=GRAD_RTOL, atol=GRAD_RTOL * float(rgrad.abs().max()), msg=f"{ids(shape)} spectral gradient vs float64")
    # value only: the same loss bits; and the whole call again: the same bits everywhere
    rc, loss_v, stats_v, _ = spectral_call(pg, td, want_grad=False)
    L.check(rc, "bnerv_loss_fwd_bwd (value only)")
    assert torch.equal(loss_v, loss) and torch.equal(stats_v, stats)
    rc, loss2, stats2, grad2 = spectral_call(pg, td)
    L.check(rc, "bnerv_loss_fwd_bwd (second run)")
    assert torch.equal(loss2, loss) and torch.equal(stats2, stats) and torch.equal(grad2, grad)


# ------------------------------------------------------------------------------------------ (a) the spectral term alone, main instantiation
@pytest.mark.parametrize("shape", R.MAIN_CASES, ids=ids)
def test_spectral_term_against_float64(ops, shape):
    check_pure_spectral(ops, shape, "main ")


# ------------------------------------------------------------------------------------------------------------- (b) through the operators
def check_operator(ops, shape, lt, ref_fn):
    pred, tgt, _, _ = inputs(shape)
    p64 = pred.double().requires_grad_(True)
    ref = ref_fn(p64, tgt.double())
    rgrad, = torch.autograd.grad(ref, [p64])
    pg, td = pred.to(DEV).requires_grad_(True), tgt.to(DEV)
    loss, stats = ops.loss_with_stats(pg, td, lt)
    ggrad, = torch.autograd.grad(loss, [pg])
    print(f"\n{lt} {ids(shape)}: loss {loss.item():.8f} f64 {ref.item():.8f}; max|grad - f64| {float((ggrad.cpu().double() - rgrad).abs().max()):.3e} "
          f"of max|grad| {float(rgrad.abs().max()):.3e}")
    assert abs(loss.item() - ref.item()) <= VAL_RTOL * abs(ref.item()), (loss.item(), ref.item())
    close(ggrad, rgrad, rtol=GRAD_RTOL, atol=GRAD_RTOL * float(rgrad.abs().max()), msg=f"{lt} {ids(shape)} grad vs float64")
    l2, st2, g2 = ops.loss_value_grad_stats(pg, td, lt)
    assert l2.item() == loss.item() and torch.equal(g2, ggrad) and torch.equal(st2, stats)


@pytest.mark.parametrize("shape", R.OPERATOR_CASES + R.LONG_ROW_CASES, ids=ids)
def test_l1_freq_operator_against_float64(ops, shape):
    """(The long rows are here for the adjoint row pass's `accumulate`: it adds the spectral gradient to the L1 gradient that is already in
    `grad`, loaded in one batch up to W = 2560 and batch by batch beyond.  In the pure spectral call above that gradient is all zeros, and a
    pass that added the wrong batch would add the same zeros.)"""
    check_operator(ops, shape, "L1_freq", lambda p, t: (60 * (p - t).abs().flatten(1).mean(1) + R.spectral_loss_f64(p, t)).mean())


@pytest.mark.parametrize("shape", R.SSIM_CASES, ids=ids)
def test_l1_ssim_freq_operator_against_float64(ops, shape):
    """The instantiation with 37-entry register arrays (bnerv_loss_ssim_fwd_bwd)."""
    check_operator(ops, shape, "L1_ssim_freq", lambda p, t: loss_f64(p, t, "L1_ssim_freq"))


def test_a_prime_factor_beyond_the_radix_limit_is_refused(ops):
    from boosting_nerv_amd._lib import BnervError
    x = torch.rand(1, 1, 22, 74, device=DEV)                              # 74 = 2 * 37
    with pytest.raises(BnervError, match="prime factor > 31"):
        ops.loss_with_stats(x.clone().requires_grad_(True), x, "L1_freq")
    x = torch.rand(1, 1, 22, 41, device=DEV)
    with pytest.raises(BnervError, match="prime factor > 37"):
        ops.loss_with_stats(x.clone().requires_grad_(True), x, "L1_ssim_freq")


# ----------------------------------------------------------------------------------------------------------------- (c) the size limit
# A block has 160 KB of LDS and a frame is accepted when its dynamic bytes fit NEXT TO the static bytes of every kernel that may carry the
# body (DESIGN.md has the reading, kernel by kernel).  Rows: 20 W bytes + 1488 (loss_head) -> W <= 8117; columns: 40 H bytes + 48 (loss_mid)
# -> H <= 4094.  8192 and 4096, which the dynamic bytes alone would admit, are refused.  Of the lengths below the limits that factor into
# primes <= 31, 8000 and 4000 are round ones near the top; 8232 = 8 * 3 * 7^3 and 4116 = 4 * 3 * 7^3 factor too, and their dynamic bytes alone
# exceed the block.
@pytest.mark.parametrize("shape", R.LIMIT_CASES, ids=ids)
def test_largest_accepted_frames_against_float64(ops, shape):
    check_pure_spectral(ops, shape, "limit")


@pytest.mark.parametrize("shape", [(1, 1, 4, 8232), (1, 1, 4116, 4), (1, 1, 4, 8192), (1, 1, 4096, 4)], ids=ids)
def test_a_frame_beyond_the_lds_is_refused_before_anything_runs(ops, shape):
    from boosting_nerv_amd import _lib as L
    ops.prepare_loss(shape[2], shape[3])                                   # (the tables exist: the refusal is about the size alone)
    g = torch.Generator().manual_seed(R.case_seed(shape))
    tgt = torch.rand(shape, generator=g).to(DEV)
    pred = tgt + 0.1 * torch.randn(shape, generator=g).to(DEV)
    for want_grad in (True, False):
        rc, loss, stats, grad = spectral_call(pred, tgt, want_grad)
        assert rc != 0
        msg = L.load().bnerv_last_error().decode()
        assert f"{shape[2]}x{shape[3]}" in msg and "LDS" in msg, msg
        assert bool((loss == FILL).all()) and bool((stats == FILL).all()) and (grad is None or bool((grad == FILL).all()))
