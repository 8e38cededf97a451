"""Measure global magnitude pruning (prune.py, csrc/prune.hip), in ONE process:
  select   on the C1 (NeRV_Boost 1.5M) and C3 (HNeRV_Boost 3M) parameter sets: GPU time of the select (bnerv_kth_abs: memset + 8 launches),
           of the mask build (bnerv_prune_masks) and of bnerv_mask_mul over four state tensors per parameter (Adan's), HIP events, and
           torch.kthvalue on the concatenated magnitudes on the same device for scale;
  step     the C1 captured step with the gradient-mask launch (TrainStep(prune=Pruner) after an event to 40 %) against its unmasked twin
           (TrainStep(prune=None)), alternated over `--repeats` rounds of `--steps` steps, host clock around work that ends in a device
           synchronisation; the mask launch alone from a replayed graph of 50 launches;
  train    a short C1 schedule (synthetic clip, `--frames` frames, `--epochs` epochs) at final sparsity 0 / 0.2 / 0.4, events at 1/4 and 1/2
           of the run: end PSNR (fp32 and 8-bit twin), bits per parameter of the Huffman report, size of the .bnrq file.
  sparse   (only on request) the schedule of `train` at 0 / 0.2 / 0.4 / 0.8 with --bitstream_sparse: the .bnrz file of the sparse twin from the
           training run and the .bnrq file of the dense twin from --eval_only on the same checkpoint; sizes, bits per parameter, PSNR of both.
usage: python tools/kprune.py [--only select|step|train|sparse] [--steps 100] [--repeats 3] [--frames 8] [--epochs 40]   (needs the GPU)"""
import argparse
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
H, W, N_FRAMES = 720, 1280, 4


def _gpu_ms(fn, reps, before=None):
    import torch
    best = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1))
    return min(best), sum(best) / len(best)


def select(name):
    import torch
    import bench
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.prune import Pruner
    dev = torch.device("cuda:0")
    model = bench.build(name)[1].to(dev)
    pr = Pruner(model)
    params = [p.data for _, p in pr.named]
    masks = [pr.masks[n] for n, _ in pr.named]
    saved = [p.clone() for p in params]
    table = ops.PruneTable(params, masks, "kprune")
    k = int(round(0.4 * pr.n))
    out = table.kth_abs(k)
    torch.cuda.synchronize()
    mags = torch.cat([p.abs().reshape(-1) for p in params])
    want = torch.kthvalue(mags, k).values
    assert out[0:1].view(torch.float32).item() == want.item(), "select disagrees with torch.kthvalue"
    sel = _gpu_ms(lambda: table.kth_abs(k, out=out), 10)
    ref = _gpu_ms(lambda: torch.kthvalue(torch.cat([p.abs().reshape(-1) for p in params]), k), 5)

    def restore():
        for p, s in zip(params, saved):
            p.copy_(s)
    build = _gpu_ms(lambda: table.prune_masks(out), 5, before=restore)
    states = [torch.randn_like(p) for p in params for _ in range(4)]
    st_table = ops.PruneTable(states, [m for m in masks for _ in range(4)], "kprune")
    mul = _gpu_ms(st_table.mask_mul, 5)
    print(f"{name}: prunable set {pr.n} weights in {len(params)} tensors ({table.n_blocks} blocks), k = {k}")
    print(f"{name}: select {sel[0] * 1e3:.1f} us best / {sel[1] * 1e3:.1f} us mean of 10;  torch.kthvalue(cat(|w|)) {ref[0] * 1e3:.1f} us best of 5")
    print(f"{name}: mask build {build[0] * 1e3:.1f} us best of 5;  mask_mul over 4 state tensors per parameter {mul[0] * 1e3:.1f} us best of 5")
    print(f"{name}: pruned {int(out[2:4].view(torch.int64).item())} at tau {out[0:1].view(torch.float32).item():.6e}")


def step(steps, repeats):
    import torch
    import bench
    from kinpaint import time_launch
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.optimizer import Adan
    from boosting_nerv_amd.prune import Pruner
    from boosting_nerv_amd.synth import SyntheticVideo
    dev = torch.device("cuda:0")
    args = bench.build("c1")[0]
    vid = SyntheticVideo(N_FRAMES, H, W)
    frames = torch.stack([vid.frame(i, device=dev) for i in range(N_FRAMES)])
    norm = torch.tensor([(i + 1) / N_FRAMES for i in range(N_FRAMES)], dtype=torch.float64, device=dev)
    m_p, m_c = bench.build("c1")[1].to(dev), bench.build("c1")[1].to(dev)
    o_p, o_c = Adan(m_p.parameters(), lr=args.lr), Adan(m_c.parameters(), lr=args.lr)
    pr = Pruner(m_p, o_p)
    s_p = TrainStep(m_p, o_p, args.loss, False, (1, 3, H, W), dev, use_graph=True, warmup_eager=3, prune=pr)
    s_c = TrainStep(m_c, o_c, args.loss, False, (1, 3, H, W), dev, use_graph=True, warmup_eager=3)
    paths = {"masked (prune=Pruner)": s_p, "plain (prune=None)": s_c}
    for s_ in paths.values():
        for s in range(6):
            s_(frames[s % N_FRAMES:s % N_FRAMES + 1], norm[s % N_FRAMES:s % N_FRAMES + 1])
    ev = pr.prune_to(0.4)                                      # between two replays: no re-capture
    g_before = s_p.graph_a
    for s_ in paths.values():
        for s in range(6):
            s_(frames[s % N_FRAMES:s % N_FRAMES + 1], norm[s % N_FRAMES:s % N_FRAMES + 1])
    torch.cuda.synchronize()
    assert s_p.graph_a is g_before and s_c.graph_a is not None
    ms = {k: [] for k in paths}
    for r in range(repeats):
        for k, s_ in paths.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for s in range(steps):
                s_(frames[s % N_FRAMES:s % N_FRAMES + 1], norm[s % N_FRAMES:s % N_FRAMES + 1])
            torch.cuda.synchronize()
            ms[k].append((time.time() - t0) / steps * 1e3)
            print(f"c1 round {r} {k}: {ms[k][-1]:.3f} ms/step", flush=True)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    kp, kc = list(paths)
    print(f"c1 step: event to 0.4 pruned {ev['pruned']} of {ev['n']}")
    for k in paths:
        print(f"c1 step {k}: {mean[k]:.3f} ms/step (spread {max(ms[k]) - min(ms[k]):.3f} over {repeats} rounds of {steps} steps)")
    print(f"c1 step masked - plain = {(mean[kp] - mean[kc]) * 1e3:.1f} us")
    # the mask launch alone, over the gradients the last eager-looking state left: give every parameter a gradient first
    for p in m_c.parameters():
        p.grad = torch.randn_like(p)
    pr_c = Pruner(m_c, o_c)
    pr_c.prune_to(0.4)
    us = time_launch(o_c.launch_grad_mask, bracket=o_c)
    print(f"c1 added launch grad_mask_table: {us:.1f} us alone (graph of 50 launches)")


def train(frames, epochs):
    import torch
    import bench
    from boosting_nerv_amd import train_nerv_all as T
    flags = bench.RECIPES["c1"]["flags"].split()
    for drop in ("-e", "--eval_freq"):
        if drop in flags:
            i = flags.index(drop)
            del flags[i:i + 2]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for S in (0.0, 0.2, 0.4):
                tag = f"s{int(S * 100)}"
                extra = ["--data_path", f"synthetic:{frames}x{H}x{W}", "--vid", "kprune", "--outf", tag, "-e", str(epochs), "--eval_freq", str(epochs),
                         "--not_resume", "--bitstream", f"{tag}.bnrq", "-p", "1000"]
                if S > 0:
                    extra += ["--prune_sparsity", str(S), "--prune_steps", str(epochs // 4), str(epochs // 2)]
                t0 = time.time()
                T.main(flags + extra)
                torch.cuda.synchronize()
                log = open(os.path.join("output", tag, "kprune", [d for d in os.listdir(os.path.join("output", tag, "kprune"))][0], "rank0.txt")).read()
                evals = [x for x in log.splitlines() if x.startswith("Eval at epoch")]
                bpp = re.search(r"bits per parameter: ([0-9.]+)", log)
                print(f"c1 train S={S}: {time.time() - t0:.1f} s;  {evals[-1]}")
                for x in log.splitlines():
                    if x.startswith(("Prune:", "Sparsity:", "Bitstream ")):
                        print(f"c1 train S={S}: {x}")
                print(f"c1 train S={S}: bits per parameter {bpp.group(1) if bpp else '?'}, {tag}.bnrq {os.path.getsize(tag + '.bnrq')} bytes", flush=True)
        finally:
            os.chdir(cwd)


def train_sparse(frames, epochs):
    """The schedule of train() at final sparsity 0 / 0.2 / 0.4 / 0.8 with --bitstream_sparse: the training run writes the
    .bnrz file of the sparse twin, then --eval_only on its checkpoint without the flag writes the .bnrq file of the dense twin."""
    import torch
    import bench
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    flags = bench.RECIPES["c1"]["flags"].split()
    for drop in ("-e", "--eval_freq"):
        if drop in flags:
            i = flags.index(drop)
            del flags[i:i + 2]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for S in (0.0, 0.2, 0.4, 0.8):
                tag = f"z{int(S * 100)}"
                common = ["--data_path", f"synthetic:{frames}x{H}x{W}", "--vid", "kprune", "--outf", tag, "-e", str(epochs), "--eval_freq", str(epochs), "-p", "1000"]
                extra = ["--not_resume", "--bitstream", f"{tag}.bnrz", "--bitstream_sparse"]
                if S > 0:
                    extra += ["--prune_sparsity", str(S), "--prune_steps", str(epochs // 4), str(epochs // 2)]
                t0 = time.time()
                T.main(flags + common + extra)
                T.main(flags + common + ["--eval_only", "--bitstream", f"{tag}.bnrq"])
                torch.cuda.synchronize()
                out = os.path.join("output", tag, "kprune")
                log = open(os.path.join(out, os.listdir(out)[0], "rank0.txt")).read().splitlines()
                evals = [x for x in log if x.startswith("Eval at epoch")]
                print(f"c1 sparse S={S}: {time.time() - t0:.1f} s;  sparse twin: {evals[-1]}")
                for x in log:
                    if x.startswith(("Sparsity:", "Bitstream ", " bits per parameter")):
                        print(f"c1 sparse S={S}: {x}")
                for x in open(os.path.join(out, os.listdir(out)[0], "eval.txt")).read().splitlines():
                    if x.strip():
                        print(f"c1 sparse S={S}: dense twin (--eval_only): {x}")
                z, q = codec.info(f"{tag}.bnrz"), codec.info(f"{tag}.bnrq")
                print(f"c1 sparse S={S}: {tag}.bnrz {z['bytes']} bytes ({z['symbol_bits'] / z['n_symbols']:.3f} symbol bits per parameter, parse {z['zero_parse']}, "
                      f"{z['n_zero_elements']} zeros), {tag}.bnrq {q['bytes']} bytes ({q['symbol_bits'] / q['n_symbols']:.3f}); ratio {z['bytes'] / q['bytes']:.4f}", flush=True)
        finally:
            os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["select", "step", "train", "sparse"], default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=40)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kprune needs the GPU"
    if a.only in (None, "select"):
        select("c1")
        select("c3")
    if a.only in (None, "step"):
        step(a.steps, a.repeats)
    if a.only in (None, "train"):
        train(a.frames, a.epochs)
    if a.only == "sparse":
        train_sparse(a.frames, a.epochs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
