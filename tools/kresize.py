"""Times of the frame resize on one MI355X, in 32-frame chunks ([32, 3, H, W] fp32) as the loader runs it:

  (1) ops.resize_bicubic against the stock torch.nn.functional.interpolate(mode='bicubic', antialias=True) on the same GPU for
      1080p -> 720p, 1080p -> 540p and 2160p -> 1080p: outputs compared first (the derived bound of tests/test_resize_cpu.py), then HIP
      events around `--reps` back-to-back calls of each, the two alternated over `--rounds` rounds, every shape warmed up;
  (2) each pass on its own (bnerv_resize_rows, bnerv_resize_cols, events around `--reps` launches) over the HBM time of the bytes it must
      move -- rows: read B C H W, write B C H w; columns: read B C H w, write B C h w floats -- at the 6.3 TB/s a streaming copy reaches on
      this part (8 TB/s is the specification's peak);
  (3) VideoDataSet.to_device of a 64-frame 1080p 8-bit .yuv (random samples, written to a temporary directory) with and without
      --resize_list 540_960: host clock around the call, which ends in a device synchronisation, alternated.

Results go to profiles/resize.md by hand.  usage: python tools/kresize.py [--reps 20] [--rounds 3] [--out FILE.md]   (needs the GPU)"""
import argparse
import os
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (((1080, 1920), (720, 1280)), ((1080, 1920), (540, 960)), ((2160, 3840), (1080, 1920)))
HBM_ACHIEVABLE = 6.3e12      # bytes/s of a float4 streaming copy on the MI355X
CHUNK, PLANES = 32, 3


def events_ms(fn, reps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import ops, yuvio
    from boosting_nerv_amd import resize as R
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    if not torch.cuda.is_available():
        raise RuntimeError("kresize: no ROCm GPU visible")
    dev = torch.device("cuda:0")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"device: {torch.cuda.get_device_name(0)}; chunks of [{CHUNK}, {PLANES}, H, W] fp32; {a.reps} calls per window, {a.rounds} rounds, alternated")
    say()
    say("| size | max abs diff to stock | bound | resize_bicubic ms | stock interpolate ms | ratio stock / ours | rows ms (floor share) | columns ms (floor share) |")
    say("|---|---|---|---|---|---|---|---|")
    lib = L.load()
    disagree = []
    for (H, W), (h, w) in SIZES:
        x = torch.rand(CHUNK, PLANES, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(H + w))
        out = torch.empty(CHUNK, PLANES, h, w, device=dev)
        scratch = torch.empty(CHUNK * PLANES * H * w, device=dev)

        def ours():
            ops.resize_bicubic(x, (h, w), out=out, scratch=scratch)

        def stock():
            return F.interpolate(x, (h, w), mode="bicubic", align_corners=False, antialias=True).clamp_(0, 1)

        ours()
        ref = stock()
        th, tw = R.axis_table(H, h)[2], R.axis_table(W, w)[2]
        bound = (th.shape[1] + tw.shape[1] + 4) * 2.0 ** -23 * float(np.abs(th).sum(1).max() * np.abs(tw).sum(1).max())
        diff = float((out - ref).abs().max())
        if not diff <= 2 * bound:         # (both sides round in fp32 here: twice the one-sided bound of the CPU test)
            disagree.append(f"{H}x{W} -> {h}x{w}: resize_bicubic and the stock op differ by {diff:.3g} (bound {2 * bound:.3g})")
        del ref
        t_ours, t_stock = [], []
        for _ in range(a.rounds):
            t_ours.append(events_ms(ours, a.reps))
            t_stock.append(events_ms(stock, a.reps))
        tab_w, T_w, span = ops._resize_table(W, w, dev)
        tab_h, T_h, _ = ops._resize_table(H, h, dev)
        n = CHUNK * PLANES

        def rows():
            L.check(lib.bnerv_resize_rows(L.stream(), L.ptr(x), L.ptr(scratch), L.ptr(tab_w), n * H, W, w, T_w, span), "rows")

        def cols():
            L.check(lib.bnerv_resize_cols(L.stream(), L.ptr(scratch), L.ptr(out), L.ptr(tab_h), n, H, h, w, T_h, 1), "cols")

        rows(), cols()
        t_rows = min(events_ms(rows, a.reps) for _ in range(a.rounds))
        t_cols = min(events_ms(cols, a.reps) for _ in range(a.rounds))
        floor_rows = 4.0 * n * (H * W + H * w) / HBM_ACHIEVABLE * 1e3
        floor_cols = 4.0 * n * (H * w + h * w) / HBM_ACHIEVABLE * 1e3
        mo, ms = float(np.median(t_ours)), float(np.median(t_stock))
        say(f"| {H}x{W} -> {h}x{w} | {diff:.3g} | {2 * bound:.3g} | {mo:.3f} ({min(t_ours):.3f}-{max(t_ours):.3f}) | {ms:.3f} ({min(t_stock):.3f}-{max(t_stock):.3f}) "
            f"| {ms / mo:.2f} | {t_rows:.3f} ({floor_rows / t_rows:.2f}) | {t_cols:.3f} ({floor_cols / t_cols:.2f}) |")
        del x, out, scratch
        torch.cuda.empty_cache()
    say()
    say(f"floor share = (bytes the pass must move / {HBM_ACHIEVABLE / 1e12:.1f} TB/s) / measured time; the stock op's time includes its clamp_ (one more pass over the output)")
    say()
    # (3) the loader
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "noise_1920x1080_8bit.yuv")
        rng = np.random.default_rng(0)
        with open(path, "wb") as f:
            for _ in range(64):
                rng.integers(16, 236, size=yuvio.frame_samples(1080, 1920), dtype=np.uint8).tofile(f)
        sets = {"-1": VideoDataSet(SimpleNamespace(data_path=path, crop_list="1080_1920", resize_list="-1")),
                "540_960": VideoDataSet(SimpleNamespace(data_path=path, crop_list="1080_1920", resize_list="540_960"))}
        times = {k: [] for k in sets}
        for k, ds in sets.items():          # warm-up: code objects, the page cache
            ds.to_device(dev)
        for _ in range(a.rounds):
            for k, ds in sets.items():
                torch.cuda.synchronize()
                t0 = time.time()
                clip = ds.to_device(dev)
                times[k].append((time.time() - t0) * 1e3)
                del clip
        say("| to_device of 64 frames of 1080p 8-bit .yuv | ms (median, min-max) |")
        say("|---|---|")
        for k, v in times.items():
            say(f"| --resize_list {k} | {float(np.median(v)):.1f} ({min(v):.1f}-{max(v):.1f}) |")
    for text in disagree:
        say("DISAGREEMENT: " + text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if disagree:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
