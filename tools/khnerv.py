"""Time one train step of the HNeRV baseline at the Bunny 1.5M recipe ("H1": regression/bunny/hnerv.sh, fc_dim 96, 720x1280):
the captured HIP step (encoder, decoder, L2, backward, fused Adam on a resident clip) against the same step on stock PyTorch-ROCm ops
(tests/hnerv_ref.py, fp32, no TF32-style downgrade), each measurement in a FRESH child process, alternated, `--repeats` times.
Prints ms/step for both, the spread over the repeats and algorithmic FLOP over time; exits 1 if the HIP step is slower than the
stock-ops step by more than the measured spread.
usage: python tools/khnerv.py [--steps 200] [--repeats 3] [--loss L2]   (needs the GPU; `--role hip|stock` is the child form; --loss: the HIP
step's loss, e.g. Fusion6 -- the stock-ops step stays L2)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_FRAMES = 4


def step_gflop(sd):
    """algorithmic FLOP of one step's decoder convolutions: 3 x forward (forward, data gradient, weight gradient), 2 FLOP per MAC"""
    import math
    names = [k for k in sd if k.endswith("weight") and not k.startswith("encoder.") and sd[k].dim() == 4]
    h, w, total = 9, 16, 0.0
    for i, k in enumerate(names):
        co, ci, kk, _ = sd[k].shape
        total += 2.0 * co * ci * kk * kk * h * w
        if i + 1 < len(names):
            s = int(round(math.sqrt(co / sd[names[i + 1]].shape[1])))
            h, w = h * s, w * s
    return 3 * total / 1e9


def child(role, steps, loss="L2"):
    import torch
    import hnerv_ref
    from boosting_nerv_amd.model_hnerv import HNeRV
    from boosting_nerv_amd.synth import SyntheticVideo
    assert torch.cuda.is_available(), "khnerv needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    model = HNeRV(hnerv_ref.h1_args())
    vid = SyntheticVideo(N_FRAMES, 720, 1280)
    frames = torch.stack([vid.frame(i, device=dev) for i in range(N_FRAMES)])
    gf = step_gflop(model.state_dict())
    if role == "hip":
        from boosting_nerv_amd.engine import TrainStep
        from boosting_nerv_amd.optimizer import Adam
        model = model.to(dev)
        opt = Adam(model.parameters(), lr=1e-3)
        step = TrainStep(model, opt, loss, True, (1, 3, 720, 1280), dev, use_graph=True, warmup_eager=3)
        step.bind_clip(frames, torch.tensor([(i + 1) / N_FRAMES for i in range(N_FRAMES)], dtype=torch.float64, device=dev))
        run = lambda s: step.step_frame(s % N_FRAMES)
        for s in range(10):
            run(s)
        assert step.graph_a is not None
        last = lambda: float(step.psnr_out.item())
    else:
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        sd = {k: v.detach().to(dev).requires_grad_(True) for k, v in model.state_dict().items()}
        adam = hnerv_ref.AdamState(list(sd.values()), lr=1e-3)
        box = {}

        def run(s):
            box["psnr"] = hnerv_ref.train_step(sd, adam, frames[s % N_FRAMES:s % N_FRAMES + 1])[1]
        for s in range(10):
            run(s)
        last = lambda: float(box["psnr"].item())
    torch.cuda.synchronize()
    t0 = time.time()
    for s in range(steps):
        run(10 + s)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / steps * 1e3
    print(json.dumps({"role": role, "loss": loss if role == "hip" else "L2", "ms_per_step": ms, "steps": steps, "step_gflop": gf, "tflops": gf / ms, "psnr_last": last()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--role", choices=["hip", "stock"], default=None)
    ap.add_argument("--loss", default="L2", help="loss of the HIP step (the stock-ops step is always L2)")
    a = ap.parse_args()
    if a.role:
        child(a.role, a.steps, a.loss)
        return 0
    res = {"hip": [], "stock": []}
    for r in range(a.repeats):
        for role in ("hip", "stock"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--steps", str(a.steps), "--loss", a.loss], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"khnerv: the {role} child failed (exit {p.returncode}); nothing more is started")
                return 2
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            res[role].append(rec)
            print(f"repeat {r} {role:5s}: {rec['ms_per_step']:.3f} ms/step, {rec['tflops']:.1f} TFLOP/s algorithmic, last PSNR {rec['psnr_last']:.3f}", flush=True)
    hip = [x["ms_per_step"] for x in res["hip"]]
    stock = [x["ms_per_step"] for x in res["stock"]]
    spread = max(max(hip) - min(hip), max(stock) - min(stock))
    mh, ms_ = sum(hip) / len(hip), sum(stock) / len(stock)
    print(f"H1 step ({res['hip'][0]['step_gflop']:.1f} GFLOP): HIP {mh:.3f} ms (spread {max(hip) - min(hip):.3f}), stock ops {ms_:.3f} ms "
          f"(spread {max(stock) - min(stock):.3f}), ratio stock / HIP {ms_ / mh:.2f}")
    ok = mh <= ms_ + spread
    print("gate (HIP not slower than stock ops beyond the spread):", "PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
