"""Shared cases of the up-scaling decode: geometries, seeded inputs, the definition and the code rule, for
test_upscale_cpu.py (which proves that the inputs qualify for the rule) and test_gpu_upscale.py (which holds the kernels to it).

Definition: the codes of yuvio.to_yuv_reference(resize.resize_reference(x, (H, W), clamp=True), coeffs).  Nothing here comes from the code
under test."""
import functools

import numpy as np
import torch

from boosting_nerv_amd import yuvio
from boosting_nerv_amd.resize import resize_reference

# (h, w) -> (H, W): a single input pixel; W % 4 == 2 tail strips; exact 2x, non-integer and 1.5x scales; identity; a 9-tap down-sampling column
# pass next to an up-sampling row pass; several blocks; the size of the end-to-end recipe
GEOMETRIES = [((1, 1), (2, 2)), ((2, 3), (4, 6)), ((3, 5), (4, 6)), ((9, 17), (18, 34)), ((5, 7), (18, 34)), ((12, 20), (18, 30)),
              ((18, 34), (18, 34)), ((40, 30), (18, 34)), ((32, 48), (64, 96)), ((90, 160), (180, 320)), ((180, 320), (270, 480))]
IDS = [f"{h}x{w}-{H}x{W}" for (h, w), (H, W) in GEOMETRIES]
IDENTITY = 6
BATCHES = (1, 3)
DEPTHS = (8, 10)
OTHER_COLOURS = (("bt601", "full"), ("bt709", "full"))      # on OTHER_K, beside bt709 / limited on every geometry
OTHER_K = (3, 8)

TIE_WINDOW = 1e-3            # tests/test_gpu_yuv.py: in units of 2^(depth - 8) codes
TIE_SHARE = 0.015
SHARE_MIN_SAMPLES = 900      # below that a share of the samples means nothing (k = 0 .. 2)


def op_cases():
    """(k, B, depth, matrix, range) of every call the GPU test holds to the definition."""
    cases = [(k, B, depth, "bt709", "limited") for k in range(len(GEOMETRIES)) for B in BATCHES for depth in DEPTHS]
    cases += [(k, B, depth, m, r) for k in OTHER_K for B in BATCHES for depth in DEPTHS for m, r in OTHER_COLOURS]
    return cases


def case_id(case):
    k, B, depth, m, r = case
    return f"{IDS[k]}-B{B}-{depth}bit-{m}-{r}"


@functools.lru_cache(maxsize=None)
def case_input(k, B, depth):
    """x [B, 3, h, w] fp32 in [-0.1, 1.1): values outside [0, 1] and bicubic overshoot, so both clamps are hit."""
    (h, w), _ = GEOMETRIES[k]
    return torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(1000 * depth + 10 * k + B)) * 1.2 - 0.1


@functools.lru_cache(maxsize=None)
def case_resized(k, B, depth):
    """resize_reference(x, (H, W), clamp=True) as a read-only numpy array: computed once, shared."""
    a = resize_reference(case_input(k, B, depth).numpy(), GEOMETRIES[k][1], clamp=True)
    a.setflags(write=False)
    return a


def tie_split(rgb, coeffs):
    """rgb [B, 3, H, W] (the resized fp32 frame) -> (want [B, samples] int64, near [B, samples] bool): the codes of the float64 restatement and
    which samples lie within TIE_WINDOW * 2^(depth - 8) of a rounding tie."""
    B = rgb.shape[0]
    codes, pre = yuvio.to_yuv_reference(np.asarray(rgb, dtype=np.float64), coeffs, return_pre=True)
    want = np.concatenate([p.reshape(B, -1) for p in codes], axis=1).astype(np.int64)
    pre = np.concatenate([p.reshape(B, -1) for p in pre], axis=1)
    frac = pre + 0.5 - np.floor(pre + 0.5)
    return want, np.minimum(frac, 1.0 - frac) < TIE_WINDOW * 2 ** (coeffs.depth - 8)


def check_codes(got_bytes, rgb, coeffs, what=""):
    """The rule of tests/test_gpu_yuv.py::_check_codes.  got_bytes: [B, frame bytes] uint8; rgb: the resized fp32 frame of the definition.
    Codes equal wherever the float64 pre-rounding value is farther than the window from a tie, within 1 inside it."""
    B, _, H, W = rgb.shape
    want, near = tie_split(rgb, coeffs)
    got = np.ascontiguousarray(got_bytes).view(coeffs.dtype).reshape(B, -1).astype(np.int64)
    assert got.shape == want.shape == (B, yuvio.frame_samples(H, W)), (got.shape, want.shape)
    diff = np.abs(got - want)
    print(f"  {what} {B}x{H}x{W} {coeffs}: {int((diff > 0).sum())} of {diff.size} codes differ, {float(near.mean()):.4%} of the samples in the tie window")
    assert (diff[~near] == 0).all(), (what, int((diff[~near] > 0).sum()), int(diff.max()))
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
