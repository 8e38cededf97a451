"""Decoding a reduced-resolution model at the master's size, timed in ONE process with device events, no profiler:

  (a) the two-op chain  ops.resize_bicubic + ops.rgb_to_yuv420  (rows, columns, store: three launches, the full-size fp32 frame written and
      read back) against
  (b) ops.resize_to_yuv420  (rows, columns fused with the store: two launches)
      at 540x960 -> 1080x1920 and 360x640 -> 720x1280, 8 and 10 bit, into preallocated buffers: `reps` calls of each captured into a graph of
      its own, the graphs replayed in turn (tools/kdecode.py time_graph), best and worst of `rounds`.  The two are checked to write the same
      bytes first.  The operands of a replayed call stay in the last-level cache: the GB/s figures are rates of that cache, not of HBM;
  (c) the frame loop of codec.Decoder on a seeded NeRV_Boost model of 540x960 (the C1 recipe with one stage less), written as a post-hoc file
      under --resize_list 540_960 of a 1080x1920 crop: frames_yuv() without upscale, with upscale=True, and for rgb8 likewise -- host clock
      around a loop that ends in a device synchronisation, per frame, alternated, round 0 not counted.

The byte counts each form must move are printed beside the times, computed from the shapes (profiles/upscale_decode.md).

usage: python tools/kupscale.py [--rounds 5] [--reps 50] [--frames 32] [--skip_loop]   (needs the GPU)"""
import argparse
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = (((540, 960), (1080, 1920)), ((360, 640), (720, 1280)))
LOOP_FLAGS = ("--model NeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin --norm none "
              "--crop_list 1080_1920 --resize_list 540_960 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 3 2 2 --ks 0_3_3 "
              "--reduce 2 --dec_blks 1 1 2 2 --modelsize 0.8 --lower_width 12 -b 1 --quant_model_bit 8 --quant_embed_bit 6")


def traffic(h, w, H, W, bps):
    """Bytes each form must move for one frame, from the shapes: (chain, fused, the share of the chain that is the full-size fp32 frame)."""
    rows = 12 * h * w + 12 * h * W                     # the row pass: x in, the [3, h, W] intermediate out (both forms)
    packed = H * W * 3 // 2 * bps
    frame = 12 * H * W                                 # the full-size fp32 frame: written by the column pass, read back by the store
    chain = rows + 12 * h * W + frame + frame + packed
    fused = rows + 12 * h * W + packed
    return chain, fused, 2 * frame


def run_ops(rounds, reps):
    import torch
    from kdecode import time_graph
    from boosting_nerv_amd import ops, yuvio
    dev = torch.device("cuda:0")
    for (h, w), (H, W) in SHAPES:
        x = (torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)) * 1.2 - 0.1).to(dev)
        full = torch.empty(1, 3, H, W, device=dev)
        scratch = torch.empty(3 * h * W, device=dev)
        for depth in (8, 10):
            c = yuvio.coefficients("bt709", "limited", depth)
            bps = c.bytes_per_sample
            a = torch.empty(1, yuvio.frame_samples(H, W) * bps, dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)

            def chain():
                ops.rgb_to_yuv420(ops.resize_bicubic(x, (H, W), out=full, scratch=scratch), c, out=a)

            def fused():
                ops.resize_to_yuv420(x, (H, W), c, out=b, scratch=scratch)
            chain()
            fused()
            differ = int((a != b).sum().item())
            (c_lo, c_hi), (f_lo, f_hi) = time_graph([chain, fused], reps=reps, rounds=rounds)
            n_chain, n_fused, n_frame = traffic(h, w, H, W, bps)
            print(f"{h}x{w} -> {H}x{W} {depth} bit: chain {c_lo:.1f} us (worst {c_hi:.1f}; {n_chain / 1e6:.1f} MB, {n_chain / c_lo / 1e3:.0f} GB/s) | "
                  f"fused {f_lo:.1f} us (worst {f_hi:.1f}; {n_fused / 1e6:.1f} MB, {n_fused / f_lo / 1e3:.0f} GB/s) | chain / fused = {c_lo / f_lo:.2f} "
                  f"(bytes: {n_chain / n_fused:.2f}; the fp32 frame is {n_frame / 1e6:.1f} MB of the chain) | {differ} bytes differ", flush=True)


def build_file(n_frames, dev):
    """A seeded NeRV_Boost model of 540x960 as the post-hoc file a run under --resize_list 540_960 of a 1080x1920 crop writes."""
    import torch
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    args = T.build_parser().parse_args(LOOP_FLAGS.split() + ["--data_path", f"synthetic:{n_frames}x1080x1920", "--vid", "bench"])
    args.final_size, args.full_data_length, args.outf = 540 * 960, n_frames, "bench"
    args.fc_dim, _ = T.solve_fc_dim(args, args.final_size, args.full_data_length)
    torch.manual_seed(args.manualSeed)
    model = T.build_model(args).to(dev)
    _, records = T.quant_model(model, args)
    buf = io.BytesIO()
    budget = codec.encode_posthoc(model, args, records, None, buf)
    return buf.getvalue(), budget


def run_loop(rounds, n_frames):
    import torch
    from boosting_nerv_amd import codec
    dev = torch.device("cuda:0")
    blob, budget = build_file(n_frames, dev)
    paths = {}
    for pack in ("yuv420p", "yuv420p10le", "rgb8"):
        for up in (None, True):
            dec = codec.Decoder(blob, dev, pack=pack, upscale=up)
            frames = dec.frames_u8 if pack == "rgb8" else dec.frames_yuv
            paths[f"{pack} {'x'.join(str(v) for v in dec.out_hw)}{' (upscale)' if up else ''}"] = (lambda f=frames: sum(1 for _ in f(copy=False)))
    print(f"frame loop: NeRV_Boost 540x960, {n_frames} frames, file {budget['bytes']} bytes", flush=True)
    times = {k: [] for k in paths}
    for rnd in range(rounds + 1):
        for key, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[key].append((time.perf_counter() - t0) / n_frames)
    for key, v in times.items():
        print(f"frame loop: {key}: {min(v) * 1e3:.3f} ms / frame (worst {max(v) * 1e3:.3f}), decoded and copied to the host", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--skip_loop", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kupscale: no ROCm GPU visible -- nothing here can be measured without one")
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    run_ops(a.rounds, a.reps)
    if not a.skip_loop:
        run_loop(a.rounds, a.frames)


if __name__ == "__main__":
    main()
