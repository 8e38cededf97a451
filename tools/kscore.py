"""Scoring a bitstream against its raw source (codec.Decoder.score, csrc/yuv.hip), timed in ONE process on a seeded C1
model at 720p and a seeded C3-shaped model at 1080p, each written as a post-hoc file (quant_model -> codec.encode_posthoc) and scored against
a 64-frame synthetic 8-bit source stored as a raw file:

  (1) the unchanged `codec psnr` path: Decoder.frames_yuv(copy=False) and yuvio.psnr_planes on the memory-mapped source, frame by frame;
  (2) Decoder.score(msssim=False): PSNR-Y / -U / -V / -YUV alone;
  (3) Decoder.score(): with MS-SSIM-Y;
  (4) the bare frames_yuv loop: what decoding and copying every frame back costs with no scoring at all.

Host clock around work that ends in a device synchronisation, `--rounds` times each, alternated, best and worst reported per frame; round 0
warms every path up (code objects, the pinned allocator, the page cache) and is not counted.  (1) and (2) are checked to give the same integers
first.  Then the two kernels alone, one frame per call, captured `reps` times into a graph and replayed (tools/kdecode.py time_graph: HIP
events); the operands of a replayed call stay in the last-level cache, so the GB/s figures are rates of that cache, not of HBM.

usage: python tools/kscore.py [--rounds 3] [--frames 64] [--only c1|c3]   (needs the GPU)"""
import argparse
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def build_file(cfg, n_frames, video, dev):
    """The post-hoc file of the seeded bench model `cfg` for an n_frames clip (HNeRV_Boost: embeddings of the synthetic frames)."""
    import torch
    import bench
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import quant_tensor
    args, model = bench.build(cfg)
    model = model.to(dev)
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    args.full_data_length, args.final_size = n_frames, h * w
    _, records = T.quant_model(model, args)
    quant_embed = None
    if "HNeRV" in args.model:
        with torch.no_grad():
            embeds = torch.cat([model.forward_encoder(video.frame(i, device=dev)[None].contiguous()) for i in range(n_frames)], 0)
        quant_embed, _ = quant_tensor(embeds, args.quant_embed_bit)
    buf = io.BytesIO()
    budget = codec.encode_posthoc(model, args, records, quant_embed, buf)
    return buf.getvalue(), budget, args


def host_psnr(dec, ref):
    """The loop of codec._psnr without its printing."""
    from boosting_nerv_amd import yuvio
    H, W = dec.frame_hw
    top, left = (v & ~1 for v in yuvio.crop_offsets(ref.height, ref.width, H, W))
    sse = []
    for i, frame in enumerate(dec.frames_yuv(copy=False)):
        y, u, v = ref.planes(i)
        src = (y[top:top + H, left:left + W], u[top // 2:(top + H) // 2, left // 2:(left + W) // 2], v[top // 2:(top + H) // 2, left // 2:(left + W) // 2])
        one = yuvio.psnr_planes(dec.split_planes(frame), src, ref.depth)
        sse.append([one["sse_y"], one["sse_u"], one["sse_v"]])
    return sse


def run(cfg, n_frames, rounds):
    import torch
    import bench
    from kdecode import time_graph
    from boosting_nerv_amd import codec, ops, synth, yuvio
    dev = torch.device("cuda:0")
    r = bench.RECIPES[cfg]
    H, W = r["h"], r["w"]
    c = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(n_frames, H, W)
    blob, budget, args = build_file(cfg, n_frames, video, dev)
    with tempfile.TemporaryDirectory() as td:
        raw_path = os.path.join(td, f"clip_{W}x{H}_8bit.yuv")
        with open(raw_path, "wb") as f:
            for i in range(n_frames):
                f.write(ops.rgb_to_yuv420(video.frame(i, device=dev)[None].contiguous(), c)[0].cpu().numpy().tobytes())
        ref = yuvio.YuvFile(raw_path)
        dec = codec.Decoder(blob, dev, pack=ref.pix_fmt)
        print(f"{cfg}: {args.model} {H}x{W}, {n_frames} frames, file {budget['bytes']} bytes, source {os.path.getsize(raw_path) / 1e6:.0f} MB ({ref.pix_fmt})", flush=True)
        paths = {"codec psnr (host)": lambda: host_psnr(dec, ref), "score(msssim=False)": lambda: dec.score(ref, msssim=False),
                 "score()": lambda: dec.score(ref), "frames_yuv alone": lambda: sum(1 for _ in dec.frames_yuv(copy=False))}
        times = {k: [] for k in paths}
        for rnd in range(rounds + 1):
            for key, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                if rnd:
                    times[key].append((time.perf_counter() - t0) / n_frames)
                elif key == "codec psnr (host)":
                    want = got
                elif key == "score(msssim=False)":
                    assert got["sse"].tolist() == want, "the device sums differ from the host's"
                elif key == "score()":
                    print(f"{cfg}: PSNR-YUV {got['mean']['psnr_yuv']:.4f} dB, MS-SSIM-Y {got['mean']['msssim_y']:.6f} (a seeded, untrained model)", flush=True)
        base = min(times["codec psnr (host)"])
        for key, v in times.items():
            print(f"{cfg}: {key}: {min(v) * 1e3:.3f} ms / frame (worst {max(v) * 1e3:.3f}) | codec psnr / this = {base / min(v):.2f}", flush=True)
        ms, plain = min(times["score()"]), min(times["score(msssim=False)"])
        print(f"{cfg}: MS-SSIM-Y adds {(ms - plain) * 1e3:.3f} ms / frame to score(): {(ms - plain) / ms:.0%} of it", flush=True)
        # the two kernels alone
        packed = dec._launch(0)[1].clone()
        src = torch.from_numpy(ref.raw(0, 1).copy()).to(dev)
        sse, luma = torch.empty(1, 3, dtype=torch.int64, device=dev), torch.empty(1, 1, H, W, device=dev)
        fns = [lambda: ops.yuv420_sse(packed, src, 1, H, W, 1, out=sse), lambda: ops.yuv_luma_f32(src, 1, 1, H, W, out=luma)]
        (s_lo, s_hi), (l_lo, l_hi) = time_graph(fns, rounds=max(rounds, 3))
        print(f"{cfg}: yuv420_sse {s_lo:.1f} us (worst {s_hi:.1f}; memset + kernel; {2 * ref.frame_bytes / s_lo / 1e3:.0f} GB/s of its {2 * ref.frame_bytes / 1e6:.1f} MB, "
              f"cache-resident) | yuv_luma_f32 {l_lo:.1f} us (worst {l_hi:.1f}; {5 * H * W / l_lo / 1e3:.0f} GB/s of its {5 * H * W / 1e6:.1f} MB)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--only", choices=("c1", "c3"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kscore: no ROCm GPU visible -- nothing here can be measured without one")
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    for cfg in ("c1", "c3"):
        if a.only in (None, cfg):
            run(cfg, a.frames, a.rounds)


if __name__ == "__main__":
    main()
