"""Time the inpainting train step, in ONE process: for the C1 shape (NeRV_Boost 720x1280, Fusion10_freq, Adan, inpanting_center) and
the HNeRV baseline at 720p ("H1": L2, fused Adam, --clip_max_norm 1, inpanting_fixed_50)
  (a) train_nerv_all._generic_step -- eager, op by op, mask multiplies in the autograd graph, a separate psnr call, clip_grad_norm_:
      the step these recipes took before the captured step learned the mask and the clip (the function is unchanged),
  (b) engine.TrainStep(mask=..., clip_max_norm=...) captured,
  (c) engine.TrainStep captured without mask or clip (the unmasked twin),
alternated over `--repeats` rounds of `--steps` steps after a warm-up of each, host clock around work that ends in a device
synchronisation.  Prints ms/step with the spread over the rounds, (b) - (c) in us, and the GPU time of each launch (b) adds to (c) --
mask head, pred, PSNR finalize, grad, the two clip launches -- timed alone from a replayed graph of 50 launches (HIP events).
Exits 1 if (b) is slower than (a) by more than the spread.
usage: python tools/kinpaint.py [--steps 100] [--repeats 3] [--only c1|h1]   (needs the GPU)"""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_FRAMES = 4
H, W = 720, 1280


def recipe(name):
    """-> (args for _generic_step, model factory, optimizer factory, takes_image)"""
    import torch
    if name == "c1":
        import bench
        from boosting_nerv_amd.optimizer import Adan
        args, _ = bench.build("c1")
        args.inpanting, args.clip_max_norm = "inpanting_center", 0.0

        def model():
            return bench.build("c1")[1]
        return args, model, (lambda ps: Adan(ps, lr=args.lr)), False
    import hnerv_ref
    from boosting_nerv_amd.model_hnerv import HNeRV
    from boosting_nerv_amd.optimizer import Adam
    args = copy.copy(hnerv_ref.h1_args())
    args.loss, args.inpanting, args.clip_max_norm = "L2", "inpanting_fixed_50", 1.0

    def model():
        torch.manual_seed(1)
        return HNeRV(args)
    return args, model, (lambda ps: Adam(ps, lr=1e-3)), True


def time_launch(fn, reps=50, rounds=5, bracket=None):
    """us per launch of fn() on the GPU: `reps` launches captured into one graph, replayed; the best of `rounds` replays.
    bracket: an optimizer whose begin_capture() .. finish_capture() bracket the capture needs (finish_capture() uploads the descriptor
    table the captured launches read: it runs BEFORE the first replay)."""
    import torch
    from boosting_nerv_amd import _lib as L
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        if bracket is not None:
            bracket.begin_capture(clip=True)
        try:
            with L.graph_capture(g, stream=side):
                for _ in range(reps):
                    fn()
        finally:
            tables = bracket.finish_capture() if bracket is not None else None      # noqa: F841  (kept alive until the replays are done)
        torch.cuda.synchronize()
        best = None
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            best = us if best is None else min(best, us)
    torch.cuda.current_stream().wait_stream(side)
    return best


def run(name, steps, repeats):
    import torch
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import hnerv_utils as hu
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.synth import SyntheticVideo
    dev = torch.device("cuda:0")
    args, make_model, make_opt, takes_image = recipe(name)
    args.transform_func = hu.TransformInput(args)
    vid = SyntheticVideo(N_FRAMES, H, W)
    frames = torch.stack([vid.frame(i, device=dev) for i in range(N_FRAMES)])
    norm = torch.tensor([(i + 1) / N_FRAMES for i in range(N_FRAMES)], dtype=torch.float64, device=dev)
    idx = torch.arange(N_FRAMES, device=dev)
    mask = args.transform_func(frames[0:1], None)[2]
    clip = args.clip_max_norm

    m_a = make_model().to(dev)
    o_a = make_opt(m_a.parameters())
    m_b = make_model().to(dev)
    o_b = make_opt(m_b.parameters())
    m_c = make_model().to(dev)
    o_c = make_opt(m_c.parameters())
    s_b = TrainStep(m_b, o_b, args.loss, takes_image, (1, 3, H, W), dev, use_graph=True, warmup_eager=3, clip_max_norm=clip, mask=mask)
    s_c = TrainStep(m_c, o_c, args.loss, takes_image, (1, 3, H, W), dev, use_graph=True, warmup_eager=3)
    paths = {
        "a generic (eager)": lambda s: T._generic_step(m_a, o_a, None, args, frames[s % N_FRAMES:s % N_FRAMES + 1], idx[s % N_FRAMES:s % N_FRAMES + 1],
                                                       norm[s % N_FRAMES:s % N_FRAMES + 1], takes_image),
        "b captured masked": lambda s: s_b(frames[s % N_FRAMES:s % N_FRAMES + 1], norm[s % N_FRAMES:s % N_FRAMES + 1]),
        "c captured plain": lambda s: s_c(frames[s % N_FRAMES:s % N_FRAMES + 1], norm[s % N_FRAMES:s % N_FRAMES + 1]),
    }
    for fn in paths.values():                                  # warm-up: every shape, the eager steps before the capture, the capture
        for s in range(12):
            fn(s)
    torch.cuda.synchronize()
    assert s_b.graph_a is not None and s_c.graph_a is not None
    ms = {k: [] for k in paths}
    for r in range(repeats):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for s in range(steps):
                fn(s)
            torch.cuda.synchronize()
            ms[k].append((time.time() - t0) / steps * 1e3)
            print(f"{name} round {r} {k}: {ms[k][-1]:.3f} ms/step", flush=True)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    ka, kb, kc = list(paths)
    n_par = sum(p.numel() for p in m_b.parameters())
    print(f"{name}: {n_par} parameters in {len(list(m_b.parameters()))} tensors, clip_max_norm {clip}, mask {args.inpanting} "
          f"({int((mask == 0).sum())} of {mask.numel()} pixels masked)")
    for k in paths:
        print(f"{name} {k}: {mean[k]:.3f} ms/step (spread {spread[k]:.3f} over {repeats} rounds of {steps} steps)")
    print(f"{name} (a) / (b) = {mean[ka] / mean[kb]:.2f};  (b) - (c) = {(mean[kb] - mean[kc]) * 1e3:.1f} us")

    # the launches (b) adds to (c), each alone
    img = frames[0:1].contiguous()
    pred = torch.rand_like(img)
    gt_m, inp = torch.empty_like(img), (torch.empty_like(img) if takes_image else None)
    pred_m, grad = torch.empty_like(img), torch.rand_like(img)
    lib = L.load()
    nb = lib.bnerv_inpaint_ws_bytes(1, 3, H * W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    stats = torch.zeros(1, L.LOSS_STATS, device=dev)
    st = L.stream
    added = [
        ("inpaint_head" + (" (+ clamped input)" if takes_image else ""),
         lambda: L.check(lib.bnerv_inpaint_head(st(), L.ptr(img), L.ptr(mask), L.ptr(inp), L.ptr(gt_m), 1, 3, H * W))),
        ("inpaint_pred", lambda: L.check(lib.bnerv_inpaint_pred(st(), L.ptr(pred), L.ptr(img), L.ptr(mask), L.ptr(pred_m), L.ptr(ws), nb, 1, 3, H * W))),
        ("inpaint_psnr (finalize)", lambda: L.check(lib.bnerv_inpaint_psnr(st(), L.ptr(ws), nb, stats.data_ptr() + 16, L.LOSS_STATS, 1, 3, H * W))),
        ("inpaint_grad", lambda: L.check(lib.bnerv_inpaint_grad(st(), L.ptr(grad), L.ptr(mask), 1, 3, H * W))),
    ]
    total = 0.0
    for label, fn in added:
        us = time_launch(fn)
        total += us
        print(f"{name} added launch {label}: {us:.1f} us")
    # the clip pair over this model's own gradient table (the eager gradients of path (a); a huge max_norm leaves them as they are)
    us = time_launch(lambda: o_a.launch_clip(1e30), bracket=o_a)
    if clip > 0:
        total += us
    print(f"{name} added launches grad_sqsum_table + grad_scale_table (clip pair): {us:.1f} us" + ("" if clip > 0 else "  (no clip in this recipe: not in (b))"))
    print(f"{name} sum of the added launches alone: {total:.1f} us  (against (b) - (c) = {(mean[kb] - mean[kc]) * 1e3:.1f} us)")
    ok = mean[kb] <= mean[ka] + max(spread[ka], spread[kb])
    print(f"{name} gate ((b) not slower than (a) beyond the spread):", "PASS" if ok else "FAIL")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["c1", "h1"], default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kinpaint needs the GPU"
    ok = True
    for name in ([a.only] if a.only else ["c1", "h1"]):
        ok = run(name, a.steps, a.repeats) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
