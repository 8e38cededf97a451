"""Raw YUV 4:2:0 in and out on the HIP path (csrc/yuv.hip, boosting_nerv_amd/yuvio.py), timed in ONE process:

  (1) bnerv_yuv420_to_rgb and bnerv_rgb_to_yuv420 at 720p and 1080p, 8 and 10 bit, one frame per call, each against a stock-torch
      restatement of the same conversion on the same GPU (index tensors and coefficient tensors prepared outside the timed region).  Both
      sides are captured `reps` times into a graph and replayed, alternated over the rounds (tools/kdecode.py time_graph: HIP events; a
      Python-driven launch costs more host time than either takes on the GPU); outputs are compared first.  The operands of a replayed
      conversion (at most 31 MB) stay in the last-level cache: the GB/s figures are rates of that cache, not of HBM.
  (2) wall time of YuvFile.to_device for a 64-frame 1080p 8-bit clip against the present path for the same frames: PIL decode of
      64 PNGs, ToTensor, torch.stack, one upload (hnerv_utils.VideoDataSet.to_device).  Host clock around work that ends in a device
      synchronisation; each side runs `--rounds` times, alternated; the files are written to a temporary directory first (not timed) and
      are in the page cache for both sides.

usage: python tools/kyuv.py [--rounds 3] [--frames 64] [--only kernels|loader]   (needs the GPU)"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


class TorchChain:
    """The two conversions as stock torch ops for one frame size and one set of coefficients."""

    def __init__(self, coeffs, H, W, dev):
        import torch
        self.c, self.H, self.W = coeffs, H, W
        self.sample = torch.uint8 if coeffs.depth == 8 else torch.int16          # (codes <= 1023: the sign bit is never set)
        f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)        # noqa: E731
        yy, xx = torch.arange(H, device=dev), torch.arange(W, device=dev)
        self.j = yy >> 1
        self.n = torch.where(yy % 2 == 0, (self.j - 1).clamp(min=0), (self.j + 1).clamp(max=H // 2 - 1))
        self.i = xx >> 1
        self.i2 = torch.where(xx % 2 == 1, (self.i + 1).clamp(max=W // 2 - 1), self.i)
        self.off = f32(coeffs.offset).view(1, 3, 1, 1)
        self.inv = f32(1.0 / coeffs.denom).view(1, 3, 1, 1)
        self.den = f32(coeffs.denom).view(1, 3, 1, 1)
        self.to_rgb, self.to_yuv = f32(coeffs.to_rgb), f32(coeffs.to_yuv)

    def load(self, raw):
        import torch
        H, W = self.H, self.W
        s = raw.view(self.sample).view(raw.shape[0], -1)
        B, hw, q = s.shape[0], H * W, (H // 2) * (W // 2)
        y = s[:, :hw].reshape(B, 1, H, W).float()
        c = s[:, hw:].reshape(B, 2, H // 2, W // 2).float()
        cv = 0.75 * c[:, :, self.j, :] + 0.25 * c[:, :, self.n, :]
        cu = 0.5 * (cv[..., self.i] + cv[..., self.i2])
        norm = (torch.cat([y, cu], 1) - self.off) * self.inv
        return torch.einsum("ck,bkhw->bchw", self.to_rgb, norm).clamp(0, 1)

    def store(self, x):
        import torch
        B = x.shape[0]
        v = torch.einsum("pc,bchw->bphw", self.to_yuv, x.clamp(0, 1))
        c = v[:, 1:]
        even, odd = c[..., 0::2], c[..., 1::2]
        left = torch.cat([even[..., :1], odd[..., :-1]], -1)
        h = (left + 2.0 * even + odd) / 4.0
        cc = 0.5 * (h[:, :, 0::2] + h[:, :, 1::2])

        def code(t, p):
            return torch.floor(self.off[:, p:p + 1] + self.den[:, p:p + 1] * t + 0.5).clamp(0, self.c.maxcode).to(self.sample).reshape(B, -1)
        return torch.cat([code(v[:, 0:1], 0), code(cc[:, 0:1], 1), code(cc[:, 1:2], 2)], 1).view(torch.uint8)


def run_kernels(rounds):
    import torch
    from kdecode import time_graph
    from boosting_nerv_amd import ops, yuvio
    dev = torch.device("cuda:0")
    slower = []
    for name, (H, W) in (("720p", (720, 1280)), ("1080p", (1080, 1920))):
        for depth in (8, 10):
            c = yuvio.coefficients("bt709", "limited", depth)
            chain = TorchChain(c, H, W, dev)
            x = (torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1)) * 1.2 - 0.1).to(dev)
            raw = ops.rgb_to_yuv420(x, c)                                      # a frame of plausible samples
            frame_bytes = raw.shape[1]
            # outputs first: the load within the tolerance of the GPU tests, the store within a code (ties) on a small share of the samples
            rgb_k, rgb_t = ops.yuv420_to_rgb(raw, c, 1, H, W), chain.load(raw)
            err = (rgb_k - rgb_t).abs().max().item()
            assert err <= 4e-6, err
            codes_t = chain.store(x)
            diff = (raw.view(chain.sample).int() - codes_t.view(chain.sample).int()).abs()
            assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < 0.01, (diff.max().item(), (diff > 0).float().mean().item())
            out_rgb, out_raw = torch.empty_like(rgb_k), torch.empty_like(raw)
            fns = [lambda: ops.yuv420_to_rgb(raw, c, 1, H, W, out=out_rgb), lambda: chain.load(raw),
                   lambda: ops.rgb_to_yuv420(x, c, out=out_raw), lambda: chain.store(x)]
            (l_lo, l_hi), (tl_lo, tl_hi), (s_lo, s_hi), (ts_lo, ts_hi) = time_graph(fns, rounds=max(rounds, 3))
            nbytes = 12 * H * W + frame_bytes
            for what, (k_lo, k_hi, t_lo, t_hi) in (("yuv420_to_rgb", (l_lo, l_hi, tl_lo, tl_hi)), ("rgb_to_yuv420", (s_lo, s_hi, ts_lo, ts_hi))):
                print(f"{what} {name} {c.pix_fmt}: kernel {k_lo:.1f} us (worst {k_hi:.1f}; {nbytes / k_lo / 1e3:.0f} GB/s of its {nbytes / (H * W):.1f} B/pixel, "
                      f"operands cache-resident) | torch chain {t_lo:.1f} us (worst {t_hi:.1f}) | torch / kernel = {t_lo / k_lo:.2f}"
                      + ("   ** the kernel is SLOWER **" if k_lo > t_lo else ""), flush=True)
                if k_lo > t_lo:
                    slower.append(f"{what} {name} {c.pix_fmt}")
            print(f"  outputs: load max |kernel - torch| {err:.2e}; store {int((diff > 0).sum().item())} of {diff.numel()} codes differ by 1", flush=True)
    return slower


def run_loader(n_frames, rounds):
    import numpy as np
    import torch
    from types import SimpleNamespace
    from PIL import Image
    from boosting_nerv_amd import ops, synth, yuvio
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    c = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(n_frames, H, W)
    with tempfile.TemporaryDirectory() as td:
        raw_path, png_dir = os.path.join(td, f"clip_{W}x{H}_8bit.yuv"), os.path.join(td, "png")
        os.makedirs(png_dir)
        with open(raw_path, "wb") as f:
            for i in range(n_frames):
                frame = video.frame(i, device=dev)
                f.write(ops.rgb_to_yuv420(frame[None].contiguous(), c)[0].cpu().numpy().tobytes())
                arr = (frame * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
                Image.fromarray(arr).save(os.path.join(png_dir, f"frame_{i:04d}.png"), compress_level=1)
        png_bytes = sum(os.path.getsize(os.path.join(png_dir, n)) for n in os.listdir(png_dir))
        print(f"loader: {n_frames} frames of {H}x{W}: raw file {os.path.getsize(raw_path) / 1e6:.0f} MB, PNG directory {png_bytes / 1e6:.0f} MB, "
              f"resident clip {n_frames * 12 * H * W / 1e6:.0f} MB", flush=True)
        crop = f"{H}_{W}"
        yuv_ds = VideoDataSet(SimpleNamespace(data_path=raw_path, crop_list=crop))
        png_ds = VideoDataSet(SimpleNamespace(data_path=png_dir, crop_list=crop))
        times = {"yuv": [], "png": []}
        for r in range(rounds + 1):                                       # round 0 warms both paths up (code objects, the pinned allocator)
            for key, ds in (("yuv", yuv_ds), ("png", png_ds)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clip = ds.to_device(dev)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert tuple(clip.shape) == (n_frames, 3, H, W)
                if r:
                    times[key].append(dt)
                if r == 0 and key == "yuv":                                # the loaded clip is the restatement of the file
                    ref = yuvio.to_rgb_reference(*yuv_ds.yuv.planes(n_frames - 1), c)
                    err = float(np.abs(clip[-1].cpu().numpy().astype(np.float64) - ref).max())
                    assert err <= 2e-6, err
                del clip
        y, p = min(times["yuv"]), min(times["png"])
        print(f"loader: YuvFile.to_device {y * 1e3:.0f} ms (worst {max(times['yuv']) * 1e3:.0f}) | PNG decode + stack + upload {p * 1e3:.0f} ms "
              f"(worst {max(times['png']) * 1e3:.0f}) | png / yuv = {p / y:.1f}", flush=True)
    return y > p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--only", choices=("kernels", "loader"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kyuv: no ROCm GPU visible -- nothing here can be measured without one")
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    slower = run_kernels(a.rounds) if a.only in (None, "kernels") else []
    if a.only in (None, "loader"):
        if run_loader(a.frames, a.rounds):
            slower.append("YuvFile.to_device")
    print("slower than the comparison: " + (", ".join(slower) if slower else "nothing"), flush=True)


if __name__ == "__main__":
    main()
