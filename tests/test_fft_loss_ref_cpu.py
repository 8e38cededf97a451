"""CPU tests of tests/fft_loss_ref.py, the float64 reference that tests/test_gpu_fft_loss.py compares the spectral-loss kernels with: it
agrees with the real reference's stored L1_freq values, its gradient is the derivative of its value, and make_inputs leaves no spectral
component near zero on any frame the GPU tests use."""
import pytest
import torch

import fft_loss_ref as R
from conftest import load_golden

ALL_CASES = R.MAIN_CASES + R.SSIM_CASES + R.LIMIT_CASES


@pytest.mark.parametrize("shape", ALL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_make_inputs_leaves_no_component_near_zero(shape):
    pred, tgt, census = R.make_inputs(shape, R.case_seed(shape))
    assert census == 0
    assert pred.dtype == torch.float32 and tgt.dtype == torch.float32 and tuple(pred.shape) == shape
    assert R.near_zero_census(pred, tgt) == 0
    d = (pred - tgt).double()
    assert 0.05 < float(d.std()) < 0.2                      # still 0.1 * randn, a nudge and not another image


def test_the_nudge_is_needed_and_keeps_the_image_real():
    """Un-nudged seeded inputs do hold components near zero (so the census is not vacuous), and the nudged spectrum is still Hermitian:
    the inverse transform's imaginary part is rounding."""
    shape = (1, 3, 77, 91)
    g = torch.Generator().manual_seed(R.case_seed(shape))
    tgt = torch.rand(shape, generator=g, dtype=torch.float64)
    d = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    assert R.near_zero_census(tgt + d, tgt) > 0
    pred, tgt32, _ = R.make_inputs(shape, R.case_seed(shape))
    assert torch.equal(tgt32, tgt.float())
    moved = (pred.double() - (tgt + d)).abs().max().item()
    assert 0 < moved < 1e-3                                   # a few components by 2e-4 rms each: far below the 0.1 noise


def test_structural_zeros():
    assert int(R.structural_zeros(7, 9).sum()) == 1 and int(R.structural_zeros(8, 9).sum()) == 2 and int(R.structural_zeros(8, 10).sum()) == 4
    assert int(R.structural_zeros(2, 2).sum()) == 4 and int(R.structural_zeros(1, 7).sum()) == 1
    x = torch.rand(1, 1, 8, 10, dtype=torch.float64)
    c = torch.view_as_real(torch.fft.fft2(x))[0, 0]
    assert float(c[R.structural_zeros(8, 10)].abs().max()) < 1e-12


@pytest.mark.parametrize("c", [0.25, -0.4])
def test_constant_offset_gives_half_its_magnitude(c):
    t = torch.rand(2, 3, 21, 26, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    v = R.spectral_loss_f64(t + c, t)
    assert v.shape == (2,) and float((v - abs(c) / 2).abs().max()) < 1e-12


@pytest.mark.parametrize("tag", ["small", "odd"])
def test_value_against_the_real_reference(tag):
    npz = load_golden("loss.npz")
    pred, tgt = torch.from_numpy(npz[f"{tag}/pred"]).double(), torch.from_numpy(npz[f"{tag}/target"]).double()
    got = (60 * (pred - tgt).abs().flatten(1).mean(1) + R.spectral_loss_f64(pred, tgt)).mean().item()
    gold = float(npz[f"{tag}/L1_freq/loss"])
    assert abs(got - gold) <= 1e-6 * abs(gold), (got, gold)


@pytest.mark.parametrize("shape", [(2, 3, 21, 26), (1, 1, 7, 1), (1, 2, 77, 91)], ids=lambda s: "x".join(map(str, s)))
def test_gradient_is_the_derivative_of_the_value(shape):
    pred, tgt, census = R.make_inputs(shape, 5)
    assert census == 0
    p, t = pred.double(), tgt.double()
    g = R.spectral_grad_f64(p, t)
    e = torch.randn(shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    # the value is piecewise linear in pred: inside one piece the central difference is exact, and census == 0 keeps every component
    # >= 1e-4 rms = 1e-5 sqrt(HW / 2) from a kink, ten standard deviations of the 1e-6 sqrt(HW / 2) that this step moves one by
    h = 1e-6
    fd = (R.spectral_loss_f64(p + h * e, t).mean() - R.spectral_loss_f64(p - h * e, t).mean()).item() / (2 * h)
    dot = float((g * e).sum())
    assert abs(fd - dot) <= 1e-6 * abs(dot), (fd, dot)
