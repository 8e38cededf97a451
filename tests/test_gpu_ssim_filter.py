"""The SSIM / MS-SSIM filter bodies keep their bits.

tests/golden/ssim_filter_bits.npz was recorded ONCE (tools/record_ssim_bits.py) with the library of the commit before the filter bodies were
rebuilt around 16-byte window loads and 4-output strips (csrc/ssim_body.h): loss value, per-sample stats and gradient of seven small
cases, inputs by seed.  Every output pixel still sees the same operations in the same order, so the requirement is torch.equal -- no
tolerance.  The cases are the smallest that reach each path of the new bodies:

    ms_even_wide   Fusion10_freq (1, 1, 176, 224)  even pyramid, W % 4 == 0: 16-byte path, full and partial tiles, one gather per coarse cell
    ms_odd_scalar  Fusion10      (1, 1, 163, 171)  odd sides from level 0: element-wise path, padded pools, per-pixel chain
    ms_odd_deeper  Fusion10_freq (2, 3, 180, 270)  odd deeper levels, W % 4 != 0 at level 0 but == 0 below, B * C > 1 (the map stride)
    ms_unaligned   Fusion10      (1, 1, 192, 352)  W % 4 == 0 through a view 4 bytes past a 16-byte boundary: the element-wise fallback
    ss_one_tile    SSIM          (1, 3, 17, 45)    single scale: one partial tile, valid region smaller than a tile
    ss_two_tiles   SSIM          (2, 1, 33, 70)
    ss_freq        L1_ssim_freq  (1, 3, 48, 96)    single scale with the spectral term (the gradient is ADDED to the spectral one)

The gradient of ms_odd_deeper (1.17 MB) is larger than the fixture may be: the file holds its last plane raw and the SHA-256 of the whole
gradient's bytes; equal digests are equal bits.  Every other gradient is held raw.  The recorder reproduced its own file on the recording
library (`--check`), so every case is deterministic there.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_filter_bits.npz")
EXPECTED = {                      # the issue's cases: what the fixture must hold, so that a re-recorded file cannot drop one
    "ms_even_wide": ("Fusion10_freq", (1, 1, 176, 224), 0),
    "ms_odd_scalar": ("Fusion10", (1, 1, 163, 171), 0),
    "ms_odd_deeper": ("Fusion10_freq", (2, 3, 180, 270), 0),
    "ms_unaligned": ("Fusion10", (1, 1, 192, 352), 1),
    "ss_one_tile": ("SSIM", (1, 3, 17, 45), 0),
    "ss_two_tiles": ("SSIM", (2, 1, 33, 70), 0),
    "ss_freq": ("L1_ssim_freq", (1, 3, 48, 96), 0),
}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    cases = {c["name"]: c for c in json.loads(bytes(z["cases"]).decode())}
    return z, cases


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand(*shape, generator=g)
    pred = (tgt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return pred, tgt


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _place(t, shift, dev):
    if not shift:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
    return v


def test_fixture_holds_every_case(golden):
    z, cases = golden
    assert os.path.getsize(GOLDEN) < 1_000_000
    assert set(cases) == set(EXPECTED)
    for name, (lt, shape, shift) in EXPECTED.items():
        c = cases[name]
        assert (c["loss_type"], tuple(c["shape"]), c["shift"]) == (lt, shape, shift), name
        assert z[name + ".loss"].dtype == np.float32 and z[name + ".grad"].dtype == np.float32
        assert z[name + ".grad"].shape == (shape if c["keep"] == "full" else shape[2:]), name


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_loss_and_gradient_keep_the_recorded_bits(golden, name):
    from boosting_nerv_amd import _lib, ops
    z, cases = golden
    c = cases[name]
    dev = torch.device("cuda:0")
    pred, tgt = _inputs(tuple(c["shape"]), c["seed"])
    assert _sha(pred.numpy(), tgt.numpy()) == c["inputs_sha256"], "the seeded inputs are not the recorded ones"
    pd, td = _place(pred, c["shift"], dev), _place(tgt, c["shift"], dev)
    assert _lib.f32c(pd).data_ptr() == pd.data_ptr()          # the kernels see the placed operand itself, not a copy
    loss, stats, grad = ops.loss_value_grad_stats(pd, td, c["loss_type"])
    loss, stats, grad = loss.reshape(1).cpu(), stats.cpu(), grad.cpu()
    want_loss, want_stats, want_grad = (torch.from_numpy(z[f"{name}.{k}"]) for k in ("loss", "stats", "grad"))
    print(f"{name}: loss {loss.item()!r} (recorded {want_loss.item()!r})")
    assert torch.equal(loss, want_loss), (loss.item(), want_loss.item())
    assert torch.equal(stats, want_stats)
    if c["keep"] == "full":
        ndiff = int((grad != want_grad).sum())
        print(f"{name}: {ndiff} of {grad.numel()} gradient elements differ from the record")
        assert torch.equal(grad, want_grad)
    else:
        ndiff = int((grad[-1, -1] != want_grad).sum())
        print(f"{name}: {ndiff} of {want_grad.numel()} elements of the last plane differ from the record")
        assert torch.equal(grad[-1, -1], want_grad)
    assert _sha(grad.numpy()) == c["grad_sha256"]
