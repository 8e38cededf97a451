"""CPU test of the loss workspace sizes (csrc/loss.hip: make_layout): bnerv_loss_ws_bytes, bnerv_loss_ssim_ws_bytes and
bnerv_psnr_ws_bytes answer what the commit before the single make_layout answered (tests/loss_ws_answers.json, recorded from that commit's
library by tools/record_loss_ws.py over the table below).  The three queries are host arithmetic: no device is touched."""
import itertools
import json
import os

from boosting_nerv_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES, CHANNELS = (1, 2, 4), (1, 3)
FRAMES = ((11, 37), (40, 56), (161, 161), (176, 208), (177, 203), (180, 270), (720, 1280), (1080, 1920))
# the zero cases: a non-positive dimension in each place, and for the SSIM query a side of 10 (the 11-tap window needs 11)
ZERO_DIMS = ((0, 3, 176, 208), (2, 0, 176, 208), (2, 3, 0, 208), (2, 3, 176, 0), (-1, 3, 176, 208), (2, -3, 176, 208), (2, 3, -176, 208), (2, 3, 176, -208))
SSIM_ZERO_DIMS = ZERO_DIMS + ((2, 3, 10, 208), (2, 3, 176, 10), (1, 1, 10, 10))


def queries():
    """[(function name, arguments)] in the order of the recorded answers."""
    dims = [(B, Cc, H, W) for B, Cc, (H, W) in itertools.product(BATCHES, CHANNELS, FRAMES)]
    q = [("bnerv_loss_ws_bytes", d + (ms, fft)) for d in dims + list(ZERO_DIMS) for ms in (0, 1) for fft in (0, 1)]
    q += [("bnerv_loss_ssim_ws_bytes", d + (fft,)) for d in dims + list(SSIM_ZERO_DIMS) for fft in (0, 1)]
    q += [("bnerv_psnr_ws_bytes", d) for d in dims + list(ZERO_DIMS)]
    return q


def answers(lib):
    return [getattr(lib, name)(*args) for name, args in queries()]


def test_workspace_sizes_are_the_parent_commits():
    with open(os.path.join(HERE, "loss_ws_answers.json")) as f:
        want = json.load(f)
    q = queries()
    got = answers(L.load())
    assert len(q) == len(want) == 48 * 7 + 8 * 4 + 11 * 2 + 8
    bad = [(name, args, g, w) for (name, args), g, w in zip(q, got, want) if g != w]
    assert not bad, bad[:5]
    zero_dims = {"bnerv_loss_ws_bytes": ZERO_DIMS, "bnerv_loss_ssim_ws_bytes": SSIM_ZERO_DIMS, "bnerv_psnr_ws_bytes": [d for d in ZERO_DIMS if d[0] <= 0]}
    for (name, args), w in zip(q, want):        # the recorded file itself: zero exactly on the zero cases (the PSNR query reads B alone)
        assert (w == 0) == (args[:4] in zero_dims[name]), (name, args, w)
