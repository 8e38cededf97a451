"""Inpainting on the captured step, host side: the C symbols of the mask kernels and of the device-side global-norm clip, their argument
checks without a device, the step-mode decision of train_nerv_all, and the mask= argument of the loss entry points."""
import argparse
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import configs

NEW_SYMBOLS = ("bnerv_grad_sqsum_table", "bnerv_grad_scale_table", "bnerv_inpaint_head", "bnerv_inpaint_ws_bytes", "bnerv_inpaint_pred",
               "bnerv_inpaint_psnr", "bnerv_inpaint_grad")


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
    assert lib.bnerv_abi_version() == 9


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(64)        # a non-null, 8- and 16-byte aligned address that is never dereferenced: every call below fails its checks first
    # clip pair: null table / workspace / result, empty grids, fewer partials than blocks, a negative or NaN norm, a misaligned workspace
    assert lib.bnerv_grad_sqsum_table(None, None, 1, 1, one) == -1 and b"grad_sqsum_table" in lib.bnerv_last_error()
    assert lib.bnerv_grad_sqsum_table(None, one, 1, 1, None) == -1
    assert lib.bnerv_grad_sqsum_table(None, one, 0, 1, one) == -1 and lib.bnerv_grad_sqsum_table(None, one, 1, 0, one) == -1
    assert lib.bnerv_grad_sqsum_table(None, one, 1, 1, C.c_void_p(68)) == -1 and b"8-byte" in lib.bnerv_last_error()
    assert lib.bnerv_grad_scale_table(None, None, 1, 1, one, 1, 1.0, one) == -1 and b"grad_scale_table" in lib.bnerv_last_error()
    assert lib.bnerv_grad_scale_table(None, one, 1, 1, None, 1, 1.0, one) == -1
    assert lib.bnerv_grad_scale_table(None, one, 1, 1, one, 1, 1.0, None) == -1
    assert lib.bnerv_grad_scale_table(None, one, 1, 2, one, 1, 1.0, one) == -1
    assert lib.bnerv_grad_scale_table(None, one, 1, 1, one, 1, -1.0, one) == -1 and b"max_norm" in lib.bnerv_last_error()
    assert lib.bnerv_grad_scale_table(None, one, 1, 1, one, 1, float("nan"), one) == -1
    # mask kernels
    assert lib.bnerv_inpaint_head(None, None, one, None, one, 1, 3, 16) == -1 and b"inpaint_head" in lib.bnerv_last_error()
    assert lib.bnerv_inpaint_head(None, one, None, None, one, 1, 3, 16) == -1 and lib.bnerv_inpaint_head(None, one, one, None, None, 1, 3, 16) == -1
    assert lib.bnerv_inpaint_head(None, one, one, None, one, 0, 3, 16) == -1 and lib.bnerv_inpaint_head(None, one, one, None, one, 1, 3, 0) == -1
    assert lib.bnerv_inpaint_pred(None, None, one, one, one, one, 64, 1, 3, 16) == -1 and b"inpaint_pred" in lib.bnerv_last_error()
    assert lib.bnerv_inpaint_pred(None, one, one, one, one, None, 64, 1, 3, 16) == -1
    assert lib.bnerv_inpaint_pred(None, one, one, one, one, one, 8, 1, 3, 16) == -3 and b"workspace" in lib.bnerv_last_error()
    assert lib.bnerv_inpaint_psnr(None, None, 64, one, 5, 1, 3, 16) == -1 and lib.bnerv_inpaint_psnr(None, one, 64, None, 5, 1, 3, 16) == -1
    assert lib.bnerv_inpaint_psnr(None, one, 64, one, 0, 1, 3, 16) == -1
    assert lib.bnerv_inpaint_grad(None, None, one, 1, 3, 16) == -1 and lib.bnerv_inpaint_grad(None, one, None, 1, 3, 16) == -1
    # one double per (plane, block of 4096 elements)
    assert lib.bnerv_inpaint_ws_bytes(2, 3, 180 * 320) == 2 * 3 * 15 * 8 and lib.bnerv_inpaint_ws_bytes(1, 3, 13 * 17) == 3 * 8
    assert lib.bnerv_inpaint_ws_bytes(0, 3, 16) == 0 and lib.bnerv_inpaint_ws_bytes(1, 3, 0) == 0


def _args(**kw):
    a = argparse.Namespace(inpanting="none", clip_max_norm=0.0)
    a.__dict__.update(kw)
    return a


def _tiny_params():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_step_mode_is_captured_for_the_fused_optimizers_whatever_mask_or_clip():
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.optimizer import Adam, Adan
    assert T.step_mode(Adan(_tiny_params(), lr=1e-3), _args(inpanting="inpanting_center")) == "captured"
    assert T.step_mode(Adam(_tiny_params(), lr=1e-3), _args(clip_max_norm=1.0)) == "captured"
    assert T.step_mode(Adan(_tiny_params(), lr=1e-3), _args(inpanting="inpanting_fixed_50", clip_max_norm=1.0)) == "captured"
    assert T.step_mode(Adan(_tiny_params(), lr=1e-3), _args()) == "captured"
    assert T.step_mode(torch.optim.Adam(_tiny_params(), lr=1e-3), _args()) == "generic"
    assert T.step_mode(torch.optim.Adam(_tiny_params(), lr=1e-3), _args(inpanting="inpanting_center", clip_max_norm=1.0)) == "generic"


def test_loss_entry_points_accept_a_mask():
    """mask= reaches the device check (the HIP path has no CPU fallback) instead of a TypeError; the frame-size checks still come first."""
    from boosting_nerv_amd import _lib, ops
    from boosting_nerv_amd import hnerv_utils as hu
    for fn in (hu.loss_fn, ops.loss_with_stats, ops.loss_value_grad_stats):
        assert inspect.signature(fn).parameters["mask"].default is None
    assert inspect.signature(ops.loss_value_grad_stats).parameters["target_masked"].default is None
    p, t, m = torch.rand(1, 3, 16, 24), torch.rand(1, 3, 16, 24), torch.ones(16, 24)
    with pytest.raises(_lib.BnervError, match="no CPU fallback"):
        hu.loss_fn(p, t, "L2", mask=m)
    with pytest.raises(_lib.BnervError, match="no CPU fallback"):
        ops.loss_value_grad_stats(p, t, "L2", mask=m)
    with pytest.raises(NotImplementedError, match="min"):
        ops.loss_with_stats(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8), "Fusion6", mask=torch.ones(8, 8))


def test_train_step_takes_a_mask_and_no_longer_drops_the_graph_for_a_clip():
    """The constructor on a CPU device: mask=None allocates nothing new, a mask brings its static buffers, a wrong shape is refused, and
    clip_max_norm leaves use_graph alone."""
    from boosting_nerv_amd import engine
    from boosting_nerv_amd.model_nerv import NeRV_Boost
    from boosting_nerv_amd.optimizer import Adan
    torch.manual_seed(1)
    model = NeRV_Boost(1, args=configs.tiny_nerv())
    cpu = torch.device("cpu")
    mk = lambda **kw: engine.TrainStep(model, Adan(model.parameters(), lr=1e-3), "L1", False, (1, 3, 180, 320), cpu, **kw)      # noqa: E731
    plain = mk(use_graph=True, clip_max_norm=1.0)
    assert plain.use_graph and plain.clip_max_norm == 1.0 and plain.mask is None and plain.static_gtm is None and plain.static_in is None
    masked = mk(use_graph=False, mask=torch.ones(180, 320, dtype=torch.float64))
    assert masked.mask.dtype == torch.float32 and masked.static_gtm.shape == (1, 3, 180, 320) and masked.static_in is None
    with pytest.raises(ValueError, match="mask"):
        mk(mask=torch.ones(90, 320))
    opt = Adan(model.parameters(), lr=1e-3)
    assert opt.clip_out is None and hasattr(opt, "launch_clip")
