"""The single-scale SSIM losses (SSIM, Fusion1-9, L1_ssim_freq), host side: the coefficient table against the reference's own loss
values (tests/golden/loss_ssim.npz, written by tools/make_ssim_loss_goldens.py from the reference's loss_fn), the small-frame refusal
and the C symbols."""
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden

NEW_TYPES = ("SSIM", "Fusion1", "Fusion2", "Fusion3", "Fusion4", "Fusion5", "Fusion6", "Fusion7", "Fusion8", "Fusion9", "L1_ssim_freq")
SSIM_TYPES = tuple(t for t in NEW_TYPES if t not in ("Fusion7", "Fusion8"))
CASES = ("sub160", "edge", "small", "odd", "720p", "1080p")
NEW_SYMBOLS = ("bnerv_loss_ssim_ws_bytes", "bnerv_loss_ssim_prepare", "bnerv_loss_ssim_fwd_bwd", "bnerv_ssim")


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("lt", NEW_TYPES)
def test_coefficient_table_reproduces_the_reference_loss(lt, tag):
    """c . (L1, L2, 1 - SSIM, FFT terms of the reference) == the reference's loss_fn(..., lt), to 1e-6 relative."""
    from boosting_nerv_amd import ops
    npz = load_golden("loss_ssim.npz")
    c1, c2, cm, cs, cf = ops.loss_coeffs(lt)
    assert cm == 0.0 and (cs != 0.0) == (lt in SSIM_TYPES)
    terms = [float(npz[f"{tag}/term/{k}"]) for k in ("l1", "l2", "ssim", "fft")]
    val = c1 * terms[0] + c2 * terms[1] + cs * terms[2] + cf * terms[3]
    gold = float(npz[f"{tag}/{lt}/loss"])
    assert abs(val - gold) <= 1e-6 * abs(gold), (lt, tag, val, gold)


def test_golden_file_lists_every_new_type_and_case():
    npz = load_golden("loss_ssim.npz")
    assert tuple(npz["types"]) == NEW_TYPES and tuple(npz["cases"]) == CASES
    assert tuple(npz["sub160/shape"]) == (2, 3, 40, 56) and tuple(npz["edge/shape"]) == (1, 3, 11, 37)
    assert tuple(npz["720p/shape"]) == (1, 3, 720, 1280) and tuple(npz["1080p/shape"]) == (1, 3, 1080, 1920)
    assert "720p/pred" not in npz.files and "1080p/pred" not in npz.files          # seeds only at full size
    assert npz["sub160/Fusion6/grad"].shape == (2, 3, 40, 56) and npz["1080p/Fusion6/grad.idx"].shape == (512,)


@pytest.mark.parametrize("lt", SSIM_TYPES)
@pytest.mark.parametrize("shape", [(1, 3, 8, 8), (1, 3, 10, 64), (2, 3, 64, 10)])
def test_small_frames_are_declined_before_the_device_check(lt, shape):
    from boosting_nerv_amd import ops
    with pytest.raises(NotImplementedError, match="min"):
        ops.loss_with_stats(torch.rand(shape), torch.rand(shape), lt)
    with pytest.raises(NotImplementedError, match="min"):
        ops.loss_value_grad_stats(torch.rand(shape), torch.rand(shape), lt)


def test_small_frames_metric_and_plain_mixes():
    from boosting_nerv_amd import _lib, ops
    with pytest.raises(NotImplementedError):
        ops.ssim(torch.rand(1, 3, 8, 40), torch.rand(1, 3, 8, 40))
    for lt in ("Fusion7", "Fusion8"):                    # no SSIM term: no size condition, the usual device check
        with pytest.raises(_lib.BnervError, match="no CPU fallback"):
            ops.loss_with_stats(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8), lt)
    with pytest.raises(_lib.BnervError, match="no CPU fallback"):       # a large enough frame reaches the device check
        ops.loss_with_stats(torch.rand(1, 3, 11, 11), torch.rand(1, 3, 11, 11), "Fusion6")
    with pytest.raises(NotImplementedError, match="not on the HIP path"):
        ops.loss_with_stats(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32), "Fusion13")


def test_new_symbols_are_declared_bound_and_exported():
    from boosting_nerv_amd import _lib
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+BNERV_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9       # additive: the version stays
    lib = _lib.load()                                    # (binds every name of SYMBOLS: a missing export raises here)
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.bnerv_loss_ssim_ws_bytes(1, 3, 10, 64, 0) == 0 and lib.bnerv_loss_ssim_ws_bytes(1, 3, 11, 37, 0) > 0
    # level 0 only: three gradient maps + tile partials + sums, far below the MS-SSIM pyramid's workspace
    assert lib.bnerv_loss_ssim_ws_bytes(1, 3, 720, 1280, 0) < lib.bnerv_loss_ws_bytes(1, 3, 720, 1280, 1, 0)
