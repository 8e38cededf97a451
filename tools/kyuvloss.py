"""Measure the plane loss (csrc/yuv.hip bnerv_yuv420_loss), in ONE process:
  kernel   the launch pair (stream kernel + finalize) at 720p and 1080p, 8 and 10 bit, writing (accumulate off) and adding into a gradient
           (accumulate on), replayed from a captured graph of 50 calls, best of 5 replays; the bytes it has to move and the rate that makes; and
           the same loss and gradient written with stock torch ops (float planes handed to it, autograd backward), eager, HIP events, best of 10;
  step     C1's (720p) and C3's (1080p) captured step with the term (TrainStep(yuv=YuvTerm), --yuv_loss form) against the step without it
           (TrainStep(yuv=None): the code path of the parent commit), alternated over `--repeats` rounds of `--steps` steps, host clock
           around work that ends in a device synchronisation;
  train    the C1 recipe on a synthetic 720p clip written out as a raw 8-bit .yuv file (`--frames` frames, `--epochs` epochs), trained with
           --loss Fusion10_freq, the same plus --yuv_loss at `--lambdas`, and --loss YUV420; every run's post-hoc bitstream scored with
           codec.Decoder.score against the file: PSNR-Y / -U / -V / -YUV, RGB PSNR, MS-SSIM-Y.
and the MS-SSIM-Y term (bnerv_yuv_luma_pair, bnerv_loss_fwd_bwd at C = 1, bnerv_luma_grad_rgb):
  msssim-kernel  the pair kernel, the C = 1 loss call and the scatter, each replayed from a captured graph of 50 calls at 720p and 1080p, the
                 whole term, and the 3-channel Fusion10 MS-SSIM call beside them for scale;
  msssim-step    C1's and C3's captured step with YuvTerm(lam 1000, lam_ms 50) against the same YuvTerm with lam_ms = 0 (the parent's path),
                 alternated as `step` does;
  msssim-train   the `train` schedule with --yuv_msssim at `--ms_lambdas` added to its rows.
and the plane loss through the up-sampler (csrc/upyuvloss.hip, bnerv_yuv420_up_loss_fwd / _bwd):
  up-kernel  the five-launch call at 360x640 -> 720x1280 and 540x960 -> 1080x1920, 8 and 10 bit, writing, adding and value only, as `kernel`
             times its pair; beside it the same loss and gradient through stock torch ops with F.interpolate(mode='bicubic',
             align_corners=False, antialias=True) as the up-sampler (antialias=True selects the Keys cubic with a = -0.5, the filter of
             resize.py; without it torch's bicubic uses a = -0.75, another function); the bytes each form has to move;
  up-step    the captured step of the C1 recipe with one stage less (360x640) with YuvTerm(lam 1000, up=(720, 1280)) against the same step
             without the term, alternated as `step` does;
  up-train   the `train` schedule at 360x640 from the 720p master (--resize_list 360_640): --loss Fusion10_freq alone against
             + --yuv_loss LAMBDA --yuv_upscale at `--lambdas`, both scored by Decoder(upscale=True).score against the master.  One seed per row.
usage: python tools/kyuvloss.py [--only kernel|step|train|msssim-kernel|msssim-step|msssim-train|up-kernel|up-step|up-train] [--steps 100]
                                [--repeats 3] [--frames 16] [--epochs 160] [--lambdas 300 3000] [--ms_lambdas 50]
(needs the GPU)"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N_FRAMES = 4


def _raw_clip(n, h, w, depth, dev):
    """(coeffs, fp32 clip [n, 3, h, w], raw bytes [n * frame]) of the synthetic clip: packed by the store kernel, loaded back by the load kernel."""
    import torch
    from boosting_nerv_amd import ops, yuvio
    from boosting_nerv_amd.synth import SyntheticVideo
    c = yuvio.coefficients("bt709", "limited", depth)
    vid = SyntheticVideo(n, h, w)
    rgb = torch.stack([vid.frame(i, device=dev) for i in range(n)])
    raw = ops.rgb_to_yuv420(rgb, c).reshape(-1)
    return c, ops.yuv420_to_rgb(raw, c, n, h, w), raw


def _torch_form(c, raw, h, w, dev):
    """The definition with stock torch ops on float planes prepared once: f(P) -> L (B = 1, weights 6 1 1)."""
    import torch
    n = h * w
    s = raw[:n * 3 // 2 * c.bytes_per_sample].view(torch.uint8 if c.bytes_per_sample == 1 else torch.int16).float()
    y, u, v = s[:n].view(1, h, w), s[n:n + n // 4].view(1, h // 2, w // 2), s[n + n // 4:].view(1, h // 2, w // 2)
    M = torch.tensor(c.to_yuv, dtype=torch.float32, device=dev)
    o, d, m = [float(x) for x in c.offset], [float(x) for x in c.denom], float(c.maxcode)

    def f(P):
        val = torch.einsum("pc,bchw->bphw", M, P)
        L = 0.75 * (((o[0] + d[0] * val[:, 0]) - y) / m).square().mean()
        for p, src in ((1, u), (2, v)):
            cc = val[:, p]
            left = torch.cat([cc[..., :1], cc[..., 1:-1:2]], dim=-1)
            hh = (left + 2.0 * cc[..., 0::2] + cc[..., 1::2]) * 0.25
            a = o[p] + d[p] * 0.5 * (hh[:, 0::2] + hh[:, 1::2])
            L = L + 0.125 * ((a - src) / m).square().mean()
        return L
    return f


def kernel():
    import torch
    from kinpaint import time_launch
    from boosting_nerv_amd import ops
    dev = torch.device("cuda:0")
    for h, w in ((720, 1280), (1080, 1920)):
        for depth in (8, 10):
            c, clip, raw = _raw_clip(1, h, w, depth, dev)
            pred = (clip + 0.05 * torch.randn_like(clip)).contiguous()
            grad, loss = torch.zeros_like(pred), torch.zeros((), device=dev)
            write = time_launch(lambda: ops.yuv420_loss_value_grad_stats(pred, raw, c, (h, w), (0, 0)))
            add = time_launch(lambda: ops.yuv420_loss_value_grad_stats(pred, raw, c, (h, w), (0, 0), grad=grad, loss=loss))
            value = time_launch(lambda: ops.yuv420_loss_value_grad_stats(pred, raw, c, (h, w), (0, 0), need_grad=False))
            px = h * w
            b_write, b_add = px * (12 + 12 + 1.5 * c.bytes_per_sample), px * (12 + 24 + 1.5 * c.bytes_per_sample)
            f = _torch_form(c, raw, h, w, dev)
            p = pred.clone().requires_grad_(True)

            def stock():
                p.grad = None
                f(p).backward()
            for _ in range(3):
                stock()
            best = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); stock(); e1.record()
                torch.cuda.synchronize()
                best.append(e0.elapsed_time(e1) * 1e3)
            mine = ops.yuv420_loss_value_grad_stats(pred, raw, c, (h, w), (0, 0))
            rel = float((mine[2] - p.grad).abs().max() / p.grad.abs().max())
            print(f"kernel {h}x{w} {depth} bit: write {write:.1f} us ({b_write / write / 1e6:.2f} TB/s of {b_write / 1e6:.1f} MB), "
                  f"accumulate {add:.1f} us ({b_add / add / 1e6:.2f} TB/s of {b_add / 1e6:.1f} MB), value only {value:.1f} us;  "
                  f"stock torch ops fwd+bwd eager {min(best):.1f} us best of 10;  max|grad - torch grad| / max|grad| {rel:.1e}", flush=True)


UP_SHAPES = (((360, 640), (720, 1280)), ((540, 960), (1080, 1920)))
UP_FLAGS = ("--model NeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin --norm none "
            "--crop_list 720_1280 --resize_list 360_640 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 2 --ks 0_3_3 "
            "--reduce 2 --dec_blks 1 1 2 2 --modelsize 0.8 --lower_width 12 -b 1 --lr 0.003")


def up_traffic(h, w, H, W, bps, need_grad=True, accumulate=False):
    """Bytes one call has to move for one frame, from the shapes: (this form, a chain through existing ops with [3, H, W] fp32 buffers)."""
    samples = H * W * 3 // 2 * bps
    rows = 12 * h * w + 12 * h * W                                     # the row pass: P in, S out
    fwd = 12 * h * W + samples + (6 * H * W if need_grad else 0)       # S in, the samples in, the error planes out
    bwd = (6 * H * W + 8 * h * W) + (8 * h * W + 12 * h * w * (2 if accumulate else 1)) if need_grad else 0
    chain = rows + 12 * h * W + 12 * H * W + (12 * H * W + samples + 12 * H * W) + (12 * H * W + 12 * h * W) + (12 * h * W + 12 * h * w)
    return rows + fwd + bwd, chain


def up_kernel():
    import torch
    import torch.nn.functional as F
    from kinpaint import time_launch
    from boosting_nerv_amd import ops
    dev = torch.device("cuda:0")
    for (h, w), (H, W) in UP_SHAPES:
        for depth in (8, 10):
            c, clip, raw = _raw_clip(1, H, W, depth, dev)
            small = ops.resize_bicubic(clip, (h, w))
            pred = (small + 0.05 * torch.randn_like(small)).contiguous()
            grad, loss = torch.zeros_like(pred), torch.zeros((), device=dev)
            call = lambda **kw: ops.yuv420_up_loss_value_grad_stats(pred, (H, W), raw, c, (H, W), (0, 0), **kw)
            write = time_launch(lambda: call())
            add = time_launch(lambda: call(grad=grad, loss=loss))
            value = time_launch(lambda: call(need_grad=False))
            f = _torch_form(c, raw, H, W, dev)
            p = pred.clone().requires_grad_(True)

            def stock():
                p.grad = None
                f(F.interpolate(p, size=(H, W), mode="bicubic", align_corners=False, antialias=True)).backward()
            for _ in range(3):
                stock()
            best = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); stock(); e1.record()
                torch.cuda.synchronize()
                best.append(e0.elapsed_time(e1) * 1e3)
            mine = call()
            rel = float((mine[2] - p.grad).abs().max() / p.grad.abs().max())
            b_w, chain = up_traffic(h, w, H, W, c.bytes_per_sample)
            b_a, b_v = up_traffic(h, w, H, W, c.bytes_per_sample, accumulate=True)[0], up_traffic(h, w, H, W, c.bytes_per_sample, need_grad=False)[0]
            print(f"up-kernel {h}x{w} -> {H}x{W} {depth} bit: write {write:.1f} us ({b_w / write / 1e6:.2f} TB/s of {b_w / 1e6:.1f} MB), "
                  f"accumulate {add:.1f} us ({b_a / 1e6:.1f} MB), value only {value:.1f} us ({b_v / 1e6:.1f} MB); a chain through [3, H, W] fp32 "
                  f"buffers would move {chain / 1e6:.1f} MB;  stock torch ops (F.interpolate bicubic, a = -0.5) fwd+bwd eager {min(best):.1f} us best of 10;  "
                  f"max|grad - torch grad| / max|grad| {rel:.1e}", flush=True)


def up_step(steps, repeats):
    import torch
    from boosting_nerv_amd import ops
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.engine import TrainStep, YuvTerm
    from boosting_nerv_amd.optimizer import Adan
    dev = torch.device("cuda:0")
    (h, w), (H, W) = UP_SHAPES[0]
    args = T.build_parser().parse_args(UP_FLAGS.split() + ["--data_path", f"synthetic:{N_FRAMES}x{H}x{W}", "--vid", "bench"])
    args.final_size, args.full_data_length, args.outf = h * w, 132, "bench"
    args.fc_dim, _ = T.solve_fc_dim(args, args.final_size, args.full_data_length)
    c, master, raw = _raw_clip(N_FRAMES, H, W, 8, dev)
    frames = ops.resize_bicubic(master, (h, w))
    norm = torch.tensor([(i + 1) / N_FRAMES for i in range(N_FRAMES)], dtype=torch.float64, device=dev)
    idx = torch.arange(N_FRAMES, device=dev)
    paths = {}
    for key, term in (("with the term (YuvTerm, lam 1000, up)", YuvTerm(raw, c, (H, W), (0, 0), lam=1000.0, up=(H, W))), ("without (yuv=None)", None)):
        torch.manual_seed(args.manualSeed)
        model = T.build_model(args).to(dev)
        paths[key] = TrainStep(model, Adan(model.parameters(), lr=args.lr), args.loss, False, (1, 3, h, w), dev, use_graph=True, warmup_eager=3, yuv=term)

    def run(s_, s):
        k = s % N_FRAMES
        if s_.yuv is None:
            s_(frames[k:k + 1], norm[k:k + 1])
        else:
            s_(frames[k:k + 1], norm[k:k + 1], frame_idx=idx[k:k + 1])
    for s_ in paths.values():
        for s in range(8):
            run(s_, s)
    torch.cuda.synchronize()
    assert all(s_.graph_a is not None for s_ in paths.values())
    ms = {k: [] for k in paths}
    for rnd in range(repeats):
        for k, s_ in paths.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for s in range(steps):
                run(s_, s)
            torch.cuda.synchronize()
            ms[k].append((time.time() - t0) / steps * 1e3)
            print(f"up-step {h}x{w} round {rnd} {k}: {ms[k][-1]:.3f} ms/step", flush=True)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    ka, kb = list(paths)
    for k in paths:
        print(f"up-step {k}: {mean[k]:.3f} ms/step (spread {max(ms[k]) - min(ms[k]):.3f} over {repeats} rounds of {steps} steps)")
    print(f"up-step with - without = {(mean[ka] - mean[kb]) * 1e3:.1f} us ({(mean[ka] / mean[kb] - 1) * 100:.2f} %)", flush=True)


def up_train(frames, epochs, lambdas):
    import torch
    from boosting_nerv_amd import codec, yuvio
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.synth import SyntheticVideo
    (h, w), (H, W) = UP_SHAPES[0]
    c = yuvio.coefficients("bt709", "limited", 8)
    runs = [("Fusion10_freq", [])] + [(f"Fusion10_freq + {lam:g} L_up", ["--yuv_loss", f"{lam:g}", "--yuv_upscale"]) for lam in lambdas]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            vid = SyntheticVideo(frames, H, W)
            src = os.path.join(tmp, f"synth_{W}x{H}_8bit.yuv")
            yuvio.write(src, (yuvio.to_yuv_reference(vid.frame(i).numpy(), c) for i in range(frames)), c.pix_fmt)
            ref = yuvio.YuvFile(src)
            print(f"up-train: {frames} frames of the synthetic clip as {os.path.basename(src)}, trained at {h}x{w}, {epochs} epochs ({frames * epochs} steps), "
                  "one seed per row; scored at the master's size (Decoder(upscale=True).score)")
            print("| loss | PSNR-Y | PSNR-U | PSNR-V | PSNR-YUV | train s |")
            print("|---|---|---|---|---|---|")
            for k, (tag, extra) in enumerate(runs):
                out = f"u{k}"
                t0 = time.time()
                T.main(UP_FLAGS.split() + extra + ["--data_path", src, "--vid", "kyuvloss", "--outf", out, "-e", str(epochs), "--eval_freq", str(epochs),
                                                   "--not_resume", "--bitstream", f"{out}.bnrq", "-p", "100000"])
                torch.cuda.synchronize()
                secs = time.time() - t0
                m = codec.Decoder(f"{out}.bnrq", "cuda:0", pack=c.pix_fmt, upscale=True).score(ref)["mean"]
                print(f"| {tag} | {m['psnr_y']:.3f} | {m['psnr_u']:.3f} | {m['psnr_v']:.3f} | {m['psnr_yuv']:.3f} | {secs:.0f} |", flush=True)
        finally:
            os.chdir(cwd)


def msssim_kernel():
    import torch
    from kinpaint import time_launch
    from boosting_nerv_amd import ops
    dev = torch.device("cuda:0")
    for h, w in ((720, 1280), (1080, 1920)):
        c, clip, raw = _raw_clip(1, h, w, 8, dev)
        pred = (clip + 0.05 * torch.randn_like(clip)).contiguous()
        grad, loss = torch.zeros_like(pred), torch.zeros((), device=dev)
        yp, ys = ops.yuv_luma_pair(pred, raw, c, (h, w), (0, 0))
        term, _, gy = ops._loss_launch(yp, ys, (0.0, 0.0, 1.0, 0.0, 0.0), True)
        k = ops.luma_grad_consts(c)
        t_pair = time_launch(lambda: ops.yuv_luma_pair(pred, raw, c, (h, w), (0, 0)))
        t_loss = time_launch(lambda: ops._loss_launch(yp, ys, (0.0, 0.0, 1.0, 0.0, 0.0), True))
        t_write = time_launch(lambda: ops.luma_grad_rgb(gy, k, 50.0, term))
        t_add = time_launch(lambda: ops.luma_grad_rgb(gy, k, 50.0, term, grad=grad, loss=loss))
        t_term = time_launch(lambda: ops.yuv420_msssim_value_grad_stats(pred, raw, c, (h, w), (0, 0), lam=50.0, grad=grad, loss=loss))
        t_rgb = time_launch(lambda: ops.loss_value_grad_stats(pred, clip, "Fusion10"))
        px = h * w
        print(f"msssim-kernel {h}x{w}: luma pair {t_pair:.1f} us ({px * 21 / t_pair / 1e6:.2f} TB/s of {px * 21 / 1e6:.1f} MB), C = 1 loss call "
              f"{t_loss:.1f} us, scatter write {t_write:.1f} us ({px * 16 / t_write / 1e6:.2f} TB/s), scatter accumulate {t_add:.1f} us "
              f"({px * 28 / t_add / 1e6:.2f} TB/s); the whole term, accumulating {t_term:.1f} us;  Fusion10 at C = 3 {t_rgb:.1f} us", flush=True)


def step(steps, repeats, ms=False):
    import torch
    import bench
    from boosting_nerv_amd.engine import TrainStep, YuvTerm
    from boosting_nerv_amd.optimizer import Adan
    dev = torch.device("cuda:0")
    for name in ("c1", "c3"):
        r = bench.RECIPES[name]
        h, w = r["h"], r["w"]
        args = bench.build(name)[0]
        takes_image = "HNeRV_Boost" in args.model or "pe" not in args.embed
        c, frames, raw = _raw_clip(N_FRAMES, h, w, 8, dev)
        norm = torch.tensor([(i + 1) / N_FRAMES for i in range(N_FRAMES)], dtype=torch.float64, device=dev)
        idx = torch.arange(N_FRAMES, device=dev)
        paths = {}
        pair = (("with the term (yuv=YuvTerm, lam 1000)", YuvTerm(raw, c, (h, w), (0, 0), lam=1000.0)), ("without (yuv=None)", None))
        if ms:
            pair = (("with MS-SSIM-Y (YuvTerm, lam 1000, lam_ms 50)", YuvTerm(raw, c, (h, w), (0, 0), lam=1000.0, lam_ms=50.0)),
                    ("without (YuvTerm, lam 1000, lam_ms 0)", YuvTerm(raw, c, (h, w), (0, 0), lam=1000.0)))
        for key, term in pair:
            model = bench.build(name)[1].to(dev)
            opt = Adan(model.parameters(), lr=args.lr)
            paths[key] = TrainStep(model, opt, args.loss, takes_image, (1, 3, h, w), dev, use_graph=True, warmup_eager=3, yuv=term)

        def run(s_, s):
            k = s % N_FRAMES
            if s_.yuv is None:
                s_(frames[k:k + 1], norm[k:k + 1])
            else:
                s_(frames[k:k + 1], norm[k:k + 1], frame_idx=idx[k:k + 1])
        for s_ in paths.values():
            for s in range(8):
                run(s_, s)
        torch.cuda.synchronize()
        assert all(s_.graph_a is not None for s_ in paths.values())
        ms = {k: [] for k in paths}
        for rnd in range(repeats):
            for k, s_ in paths.items():
                torch.cuda.synchronize()
                t0 = time.time()
                for s in range(steps):
                    run(s_, s)
                torch.cuda.synchronize()
                ms[k].append((time.time() - t0) / steps * 1e3)
                print(f"{name} round {rnd} {k}: {ms[k][-1]:.3f} ms/step", flush=True)
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        ka, kb = list(paths)
        for k in paths:
            print(f"{name} step {k}: {mean[k]:.3f} ms/step (spread {max(ms[k]) - min(ms[k]):.3f} over {repeats} rounds of {steps} steps)")
        print(f"{name} step with - without = {(mean[ka] - mean[kb]) * 1e3:.1f} us ({(mean[ka] / mean[kb] - 1) * 100:.2f} %)", flush=True)
        del paths


def train(frames, epochs, lambdas, ms_lambdas=()):
    import torch
    import bench
    from boosting_nerv_amd import codec, yuvio
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.synth import SyntheticVideo
    h, w = 720, 1280
    flags = bench.RECIPES["c1"]["flags"].split()
    for drop in ("-e", "--eval_freq", "--loss"):
        if drop in flags:
            i = flags.index(drop)
            del flags[i:i + 2]
    c = yuvio.coefficients("bt709", "limited", 8)
    runs = [("Fusion10_freq", ["--loss", "Fusion10_freq"])]
    runs += [(f"Fusion10_freq + {lam:g} L", ["--loss", "Fusion10_freq", "--yuv_loss", f"{lam:g}"]) for lam in lambdas]
    runs += [("YUV420", ["--loss", "YUV420"])]
    if ms_lambdas:
        runs = [runs[0]]
        for ms in ms_lambdas:
            runs += [(f"Fusion10_freq + {ms:g} L_ms", ["--loss", "Fusion10_freq", "--yuv_msssim", f"{ms:g}"])]
            runs += [(f"Fusion10_freq + {lam:g} L + {ms:g} L_ms", ["--loss", "Fusion10_freq", "--yuv_loss", f"{lam:g}", "--yuv_msssim", f"{ms:g}"]) for lam in lambdas]
            runs += [(f"YUV420 + {ms:g} L_ms", ["--loss", "YUV420", "--yuv_msssim", f"{ms:g}"])]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            vid = SyntheticVideo(frames, h, w)
            src = os.path.join(tmp, f"synth_{w}x{h}_8bit.yuv")
            yuvio.write(src, (yuvio.to_yuv_reference(vid.frame(i).numpy(), c) for i in range(frames)), c.pix_fmt)
            ref = yuvio.YuvFile(src)
            print(f"train: {frames} frames of the synthetic clip as {os.path.basename(src)}, {epochs} epochs ({frames * epochs} steps)")
            print("| loss | PSNR-Y | PSNR-U | PSNR-V | PSNR-YUV | PSNR-RGB | MS-SSIM-Y | train s |")
            print("|---|---|---|---|---|---|---|---|")
            for k, (tag, extra) in enumerate(runs):
                out = f"r{k}"
                t0 = time.time()
                T.main(flags + extra + ["--data_path", src, "--vid", "kyuvloss", "--outf", out, "-e", str(epochs), "--eval_freq", str(epochs), "--not_resume",
                                        "--bitstream", f"{out}.bnrq", "-p", "100000"])
                torch.cuda.synchronize()
                secs = time.time() - t0
                m = codec.Decoder(f"{out}.bnrq", "cuda:0", pack=c.pix_fmt).score(ref, rgb=True)["mean"]
                print(f"| {tag} | {m['psnr_y']:.3f} | {m['psnr_u']:.3f} | {m['psnr_v']:.3f} | {m['psnr_yuv']:.3f} | {m['psnr_rgb']:.3f} | {m['msssim_y']:.5f} | {secs:.0f} |",
                      flush=True)
        finally:
            os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernel", "step", "train", "msssim-kernel", "msssim-step", "msssim-train", "up-kernel", "up-step", "up-train"],
                    default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=160)
    ap.add_argument("--lambdas", type=float, nargs="+", default=[300.0, 3000.0])
    ap.add_argument("--ms_lambdas", type=float, nargs="+", default=[50.0])
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel()
    if a.only in (None, "step"):
        step(a.steps, a.repeats)
    if a.only in (None, "train"):
        train(a.frames, a.epochs, a.lambdas)
    if a.only == "msssim-kernel":
        msssim_kernel()
    if a.only == "msssim-step":
        step(a.steps, a.repeats, ms=True)
    if a.only == "msssim-train":
        train(a.frames, a.epochs, a.lambdas, a.ms_lambdas)
    if a.only == "up-kernel":
        up_kernel()
    if a.only == "up-step":
        up_step(a.steps, a.repeats)
    if a.only == "up-train":
        up_train(a.frames, a.epochs, a.lambdas)


if __name__ == "__main__":
    main()
