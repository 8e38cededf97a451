"""Per-call time of one loss type (value + gradient) inside a captured graph, or of the stock PyTorch restatement of the SSIM losses:
    python tools/kssim.py --type Fusion6 --size 720p [--lib PATH] [--stock] [--calls N] [--trace]
Prints one JSON line.  A captured graph holds 20 calls; the figure is the median over replays of (replay time / 20), device events.
--stock: forward + backward of the same loss through stock ops (oracle.msssim_ref.ssim on device tensors), eager, median per call.
--trace: a few eager calls and nothing else -- the program for rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SSIM_ENTRY_POINTS = ("bnerv_loss_ssim_ws_bytes", "bnerv_loss_ssim_prepare", "bnerv_loss_ssim_fwd_bwd", "bnerv_ssim")
SIZES = {"720p": (720, 1280), "1080p": (1080, 1920)}
STOCK = {"Fusion6": (0.7, 0.3, 0.0), "L1_ssim_freq": (42.0, 18.0, 1.0), "SSIM": (0.0, 1.0, 0.0)}      # c_l1, c_ss, c_fft


def stock_loss(pred, tgt, lt):
    from oracle import msssim_ref
    c1, cs, cf = STOCK[lt]
    loss = cs * (1 - msssim_ref.ssim(pred, tgt, data_range=1, size_average=False))
    if c1:
        loss = loss + c1 * (pred - tgt).abs().flatten(1).mean(1)
    if cf:
        loss = loss + cf * torch.view_as_real(torch.fft.fft2(pred) - torch.fft.fft2(tgt)).abs().flatten(1).mean(1)
    return loss.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--type", default="Fusion6")
    ap.add_argument("--size", default="720p", choices=sorted(SIZES))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--stock", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=60)
    a = ap.parse_args()
    if a.lib:
        os.environ["BNERV_LIB"] = os.path.abspath(a.lib)
    from boosting_nerv_amd import _lib, ops
    _lib.load(optional=SSIM_ENTRY_POINTS)                    # (--lib may name a build that predates them)
    dev = torch.device("cuda:0")
    H, W = SIZES[a.size]
    g = torch.Generator().manual_seed(6)
    tgt = torch.rand(1, 3, H, W, generator=g)
    pred = (tgt + 0.1 * torch.randn(tgt.shape, generator=g)).clamp(0, 1).to(dev)
    tgt = tgt.to(dev)
    rec = {"type": a.type, "size": a.size, "lib": a.lib or "default", "mode": "stock" if a.stock else "trace" if a.trace else "graph"}
    if a.trace:
        for _ in range(5):
            ops.loss_value_grad_stats(pred, tgt, a.type)
        torch.cuda.synchronize()
        print(json.dumps(rec))
        return
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    times = []
    if a.stock:
        p = pred.clone().requires_grad_(True)
        for it in range(10 + a.replays):
            s, e = ev(), ev()
            s.record()
            torch.autograd.grad(stock_loss(p, tgt, a.type), [p])
            e.record()
            torch.cuda.synchronize()
            if it >= 10:
                times.append(s.elapsed_time(e) * 1e3)
    else:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                out = ops.loss_value_grad_stats(pred, tgt, a.type)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with _lib.graph_capture(graph, stream=side):
                for _ in range(a.calls):
                    out = ops.loss_value_grad_stats(pred, tgt, a.type)
        for it in range(10 + a.replays):
            s, e = ev(), ev()
            s.record()
            graph.replay()
            e.record()
            torch.cuda.synchronize()
            if it >= 10:
                times.append(s.elapsed_time(e) * 1e3 / a.calls)
        rec["loss"] = out[0].item()
    rec.update(us_median=round(statistics.median(times), 2), us_min=round(min(times), 2), us_max=round(max(times), 2), n=len(times))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
