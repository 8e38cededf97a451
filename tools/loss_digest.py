"""Digest of loss value and gradient of the loss types a library builds, on the loss.npz inputs (small, odd) and a seeded 720p frame:
    python tools/loss_digest.py [--lib PATH] [--types L1 L2 ...] > digest.txt
One line per (type, case): sha256[:16] over the bytes of the loss scalar, the per-sample statistics and the gradient, then the loss.  Run on
two builds (--lib another libbnerv_hip.so of the same ABI; the SSIM entry points may be missing there) and diff the outputs: equal
digests = equal bits.  profiles/ssim_loss_digest.txt holds such a pair."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SSIM_ENTRY_POINTS = ("bnerv_loss_ssim_ws_bytes", "bnerv_loss_ssim_prepare", "bnerv_loss_ssim_fwd_bwd", "bnerv_ssim")
EXISTING = ("L1", "L2", "L1_freq", "Fusion10", "Fusion11", "Fusion12", "Fusion10_freq")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--types", nargs="+", default=list(EXISTING))
    a = ap.parse_args()
    if a.lib:
        os.environ["BNERV_LIB"] = os.path.abspath(a.lib)
    from boosting_nerv_amd import _lib, ops
    _lib.load(optional=SSIM_ENTRY_POINTS)                    # (--lib may name a build that predates them)
    dev = torch.device("cuda:0")
    npz = np.load(os.path.join(ROOT, "tests", "golden", "loss.npz"), allow_pickle=False)
    cases = [(t, torch.from_numpy(npz[f"{t}/pred"]), torch.from_numpy(npz[f"{t}/target"])) for t in ("small", "odd")]
    g = torch.Generator().manual_seed(int(npz["720p/seed"]))
    tgt = torch.rand(1, 3, 720, 1280, generator=g)
    cases.append(("720p", (tgt + 0.1 * torch.randn(tgt.shape, generator=g)).clamp(0, 1), tgt))
    for lt in a.types:
        for tag, pred, tgt in cases:
            loss, stats, grad = ops.loss_value_grad_stats(pred.to(dev), tgt.to(dev), lt)
            h = hashlib.sha256()
            for t in (loss, stats, grad):
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
            print(f"{lt:14s} {tag:6s} {h.hexdigest()[:16]}  loss {loss.item():.9g}")


if __name__ == "__main__":
    main()
