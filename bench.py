#!/usr/bin/env python
"""bench.py -- train frames/sec of the Boosting-NeRV conditional-decoder path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W       (N = 1: in this process; N > 1: re-launches itself, one rank per GPU)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W   (the driver's N > 1 form)
    python bench.py ... --full                 (also every extra object listed below: kernel roofline, parity, CPU baseline, ...)
    python bench.py ... --dump-outputs DIR     (after the timed steps: what the last timed step returned, as DIR/<name>.npy)

A "step" is one pass of the hot path over one batch: forward of the decoder, Fusion10_freq loss, backward, [one flat-bucket
RCCL all-reduce when N > 1], fused Adan -- exactly train_nerv_all.py:328-348 of the reference -- on frames already resident
in HBM.  Workload at N=1: BASELINE configs[1] = NeRV-boost 1.5M on a Bunny-shaped synthetic clip (132 x 3x720x1280), batch
1 per GPU (the reference recipe's `-b 1`; `-b N -d` on N GPUs), weak scaling.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline (value, ms_per_step, the step's algorithmic
`step_roofline`, config).  Extra objects on the line, measured only with --full:
  roofline      the conv family the step launches at the model's last stage (C -> C 3x3 at full resolution: TAT conv0 / conv1
                forwards, their data gradients, the weight gradients), each instantiation timed live with HIP events on the
                stream it is launched on; `achieved` = flop-weighted mean against the dense fp32 MFMA peak, `slowest` and the
                per-kernel list beside it
  step_roofline the whole measured step against max(flops / MFMA peak, bytes / HBM peak) of its algorithmic conv + dense work
  eval_psnr_db  pred_seen_psnr of a few frames after the timed steps
  cpu_baseline  the CPU oracle (oracle/cpu_ref.py: the reference's algorithm in plain fp32 torch) running the SAME train step
                on this box's host cores for a bounded sample (rank 0, N=1 only): 3 warm-up + up to 20 timed steps, 30 s budget
  parity, host_frames, recipe, other_configs, stock_rocm   (see main())

--dump-outputs DIR writes the arrays a caller of the timed step receives after its LAST timed step (rank 0): loss.npy, psnr.npy
(bpp.npy for c5) and param.<state_dict key>.npy for every floating-point model tensor, float32, at most 64 MB in all (a larger tensor
is replaced by a fixed seeded sample of its elements).  The inputs are seeded, so two builds run with the same arguments can be
compared file by file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

RECIPES = {
    # scripts/regression/bunny/nerv_boost.sh:4-9 (--modelsize 0.8 -> "1.5M")
    "c1": dict(n=132, h=720, w=1280, flags="--model NeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 "
               "--act sin --norm none --crop_list 720_1280 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 "
               "--dec_strds 5 2 2 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 2 2 --modelsize 0.8 -e 300 --eval_freq 30 --lower_width 12 -b 1 --lr 0.003",
               name="NeRV-boost 1.5M"),
    # scripts/regression/UVG/hnerv_boost.sh:7-12 (--modelsize 2.8 -> "3M")
    "c3": dict(n=600, h=1080, w=1920, flags="--model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 "
               "--act sin --norm none --crop_list 1080_1920 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 3 2 2 2 "
               "--enc_dim 64_16 --dec_strds 5 3 2 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 2 2 --modelsize 2.8 -e 300 --eval_freq 30 "
               "--lower_width 12 -b 1 --lr 0.003", name="HNeRV-boost 3M"),
    # scripts/regression/UVG/enerv_boost.sh:7-12 (--modelsize 1.8 -> "3M")
    "c4": dict(n=600, h=1080, w=1920, flags="--model ENeRV_Boost --sft_block res_sft --ch_t 32 --block_dim 128 --optim_type Adan "
               "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 1080_1920 --resize_list -1 --loss Fusion10_freq "
               "--embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 3 2 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 2 2 --modelsize 1.8 -e 300 "
               "--eval_freq 30 --lower_width 12 -b 1 --lr 0.0015", name="E-NeRV-boost 3M"),
    # scripts/compression/hnerv_boost.sh:7-16 (BASELINE configs[4]: the C3 model built with --quant, rate-distortion step)
    "c5": dict(n=600, h=1080, w=1920, flags="--model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 "
               "--act sin --norm none --crop_list 1080_1920 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 3 2 2 2 "
               "--enc_dim 64_16 --dec_strds 5 3 2 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 2 2 --modelsize 2.8 -e 100 --eval_freq 30 "
               "--lower_width 12 -b 1 --lr 0.0005 --lr_type cosine_0_1_0.1 --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
               "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.05 --target_bit 4",
               name="HNeRV-boost 3M, CEM compression step"),
}
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 MFMA peak (= fp32 vector peak)
PEAK_HBM_GBS = 8000.0
PEAK_BF16_MFMA_TFLOPS = 2500.0     # dense bf16 MFMA peak (no sparsity)


def build(cfg_name):
    from boosting_nerv_amd import train_nerv_all as T
    r = RECIPES[cfg_name]
    if cfg_name == "c5":
        from boosting_nerv_amd import train_nerv_compression as T5
    args = (T5 if cfg_name == "c5" else T).build_parser().parse_args(r["flags"].split() + ["--data_path", f"synthetic:{r['n']}x{r['h']}x{r['w']}", "--vid", "bench"])
    args.final_size = r["h"] * r["w"]
    args.full_data_length = r["n"]
    args.outf = "bench"
    args.fc_dim, _ = T.solve_fc_dim(args, args.final_size, args.full_data_length)
    torch.manual_seed(args.manualSeed)
    return args, T.build_model(args)


# Algorithmic work per trained frame (BASELINE.md section 3 / SURVEY 8(d): conv + dense only, train = fwd + dgrad + wgrad,
# 2 flops per MAC, every activation once in + once out per conv at 4 B)
STEP_WORK = {"c1": (58.0e9, 2.165e9), "c3": (1542e9, 16.08e9), "c4": (367.8e9, 6.42e9), "c5": (1542e9, 16.08e9)}


def _time_launches(fn, reps):
    """Average duration of one launch of `fn`, HIP events on the launch stream.  The `reps` launches are captured into a hipGraph
    and the graph is replayed (as the train step itself runs them): a Python-driven ctypes call costs about as much host time as
    these kernels take on the GPU (40-60 us), so an eager loop measures whichever side is slower on the day -- the same build read
    43 and 60 us for the same kernel on two boxes.  Replay leaves only kernel time, which is what the rocprofv3 kernel-trace average
    of the same instantiation reports.  (Deferred slab reductions ride on the following launch exactly as in the step; the
    leftovers are one small launch at the end of the graph.)  Falls back to the eager loop if the capture fails."""
    from boosting_nerv_amd import ops, _lib as L
    for _ in range(5):
        fn()
    ops._flush_deferred()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)   # current stream == launch stream
    torch.cuda.synchronize()
    try:
        side, ctx, g = torch.cuda.Stream(), L.new_ctx(), torch.cuda.CUDAGraph()
        with L.use_ctx(ctx):
            with L.graph_capture(g, stream=side):
                for _ in range(reps):
                    fn()
                ops._flush_deferred()
        g.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(4):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1e-3 / (4 * reps)
        del g
        return t
    except Exception as e:                                   # noqa: BLE001  (report, then measure the eager way)
        print(f"[bench] launch capture failed ({type(e).__name__}: {e}); timing the eager loop", file=sys.stderr)
        torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ops._flush_deferred()
    return e0.elapsed_time(e1) * 1e-3 / reps


def step_kernel_roofline(dev, Cc, H, W, reps=20):
    """The heavy launches of one train step at the model's LAST stage (Cc -> Cc 3x3 at HxW: two TAT blocks + one stride-1 block
    conv), each timed live with HIP events through the C-ABI exactly as ops._tat_forward / _tat_backward / _SNeRVBlock issue
    them (same prologue / epilogue modes, same auxiliary tensors -> same template instantiations as the step's trace):
        K2s  conv0 forward   [affine -> 3x3 -> bias -> gelu, gelu']      x2 per step
        K3s  conv1 forward   [affine -> 3x3 -> bias -> + residual]       x2
        K1   block conv      [3x3 -> bias -> sin, cos]                   x1
        wA|dK3s  conv1 weight gradient (affine prologue) | conv1 data grad [3x3^T -> * gelu' * (1+s), channel sums]   x2
        wA|dK2s  conv0 weight gradient (affine prologue) | conv0 data grad [3x3^T -> (dout + . (1+s)) * cos, sums]    x2
        wP|dK1   block-conv weight gradient (plain)      | block-conv data grad [3x3^T]                               x1
    (the backward launches are PAIRS since round 3: the two halves read the same gradient and run as interleaved roles of one grid,
    ops._wgrad_conv_pair -- a pair is two convolutions' flops and every distinct tensor once).
    Algorithmic work per launch: flops = 2 * Cc*Cc*9 * H*W per convolution; bytes = activations once in + once out (+ each auxiliary
    tensor the mode reads or writes) + weights, 4 B each.  At Cc = 12 the plain modes sit just above the ridge (157.3 TF / 8 TB/s =
    19.7 flop/B) and the data gradients with 3-4 auxiliary planes below it, so every row also carries its own bound
    (max of flops / MFMA peak and bytes / HBM peak) and `frac_of_own_roof`.  `achieved` of the family = sum(flops) / sum(time)
    with the per-step launch counts as weights against the dense fp32 MFMA peak; the slowest member is reported next to it."""
    from boosting_nerv_amd import ops, _lib as L
    B = 1
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dev)
    x, y0, h, gp, c0, dout = (rn(B, Cc, H, W) for _ in range(6))
    w = rn(Cc, Cc, 3, 3, sc=0.1)
    b = rn(Cc)
    sc, sh = rn(B, Cc, sc=0.1), rn(B, Cc, sc=0.1)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    kw = dict(B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3)
    plane = Cc * H * W * 4.0
    wb = Cc * Cc * 9 * 4.0
    cases = [   # name (its first word is the row key the PMC traffic profiles are matched by), launches per step, tensors moved (in planes), launcher
        ("K2s conv0 fwd: affine->conv->bias->gelu,gelu'", 2, 3, lambda: ops._conv(x, w, b, out, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_GELU, scale=sc, shift=sh, out2=out2, **kw)),
        ("K3s conv1 fwd: affine->conv->bias->+res", 2, 3, lambda: ops._conv(h, w, b, out, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_RES, scale=sc, shift=sh, aux0=y0, **kw)),
        ("K1 block conv fwd: conv->bias->sin,cos", 1, 3, lambda: ops._conv(x, w, b, out, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS_SIN, out2=out2, **kw)),
        ("wA|dK3s conv1 bwd pair: weight grad (affine) | conv^T->dgelu(saved)+sums", 2, 4, lambda: ops._wgrad_conv_pair(
            dict(x=h, g=dout, dw=dw, db=db, in_mode=L.IN_AFFINE, g_mode=L.IN_UNSHUFFLE, scale=sc, shift=sh, **kw),
            dict(x=dout, w=w, bias=None, out=out, in_mode=L.IN_PLAIN, ep_mode=L.EP_DGELU_SAVED, transposed=1, aux0=gp, aux1=h, scale=sc, **kw))),
        ("wA|dK2s conv0 bwd pair: weight grad (affine) | conv^T->dsin+sums", 2, 5, lambda: ops._wgrad_conv_pair(
            dict(x=y0, g=dout, dw=dw, db=db, in_mode=L.IN_AFFINE, g_mode=L.IN_UNSHUFFLE, scale=sc, shift=sh, **kw),
            dict(x=dout, w=w, bias=None, out=out, in_mode=L.IN_PLAIN, ep_mode=L.EP_DSIN, transposed=1, aux0=y0, aux1=gp, aux2=c0, scale=sc, **kw))),
        ("wP|dK1 block conv bwd pair: weight grad (plain) | conv^T", 1, 3, lambda: ops._wgrad_conv_pair(
            dict(x=x, g=dout, dw=dw, db=db, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE, g_s=1, **kw),
            dict(x=dout, w=w, bias=None, out=out, in_mode=L.IN_PLAIN, ep_mode=L.EP_PLAIN, transposed=1, **kw))),
    ]
    flops1 = 2.0 * Cc * Cc * 9 * H * W
    rows, tf, tt, nl = [], 0.0, 0.0, 0
    troof = 0.0
    keys = {"K2s": "k2s", "K3s": "k3s", "K1": "k1", "wA|dK3s": "pair_dk3s", "wA|dK2s": "pair_dk2s", "wP|dK1": "pair_dk1"}
    for name, n, planes, fn in cases:
        t = _time_launches(fn, reps)       # (slab reductions are deferred exactly as in the step: they ride on the following launch)
        ops._flush_deferred()
        nconv = 2 if "pair" in name else 1      # a pair is two convolutions
        flops = flops1 * nconv
        ach = flops / t / 1e12
        nbytes = planes * plane + nconv * wb
        t_m, t_h = flops / (PEAK_FP32_MFMA_TFLOPS * 1e12), nbytes / (PEAK_HBM_GBS * 1e9)
        rows.append({"kernel": name, "row": keys[name.split()[0]], "per_step": n, "avg_launch_us": round(t * 1e6, 2), "achieved": round(ach, 2), "frac": round(ach / PEAK_FP32_MFMA_TFLOPS, 4),
                     "flops_per_launch": flops, "bytes_per_launch": nbytes, "algorithmic_GB_per_s": round(nbytes / t / 1e9, 1), "bound": "mfma" if t_m >= t_h else "hbm",
                     "frac_of_own_roof": round(max(t_m, t_h) / t, 4)})
        if Cc > 16:     # the pipe these layers run on: six bf16 products per f32 product on v_mfma_f32_16x16x32_bf16
            rows[-1]["frac_of_split_pipe"] = round(ach / (PEAK_BF16_MFMA_TFLOPS / 6), 4)
        tf += n * flops
        tt += n * t
        nl += n
        troof += n * max(t_m, t_h)
    ach = tf / tt / 1e12
    slow = min(rows, key=lambda r: r["achieved"])
    # HBM bytes per launch from the PMC counters (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, gfx950 x2 FETCH
    # correction; tools/pmc_traffic.py), committed with their summaries -- bench.py cannot run under the counter collector.  A profile
    # belongs to ONE row (`row` + `shape`) and is only valid for the kernel sources it was measured on: it carries a SHA-256 of those
    # sources, and a profile whose stamp differs from the tree is refused -- `traffic` stays null rather than describing another kernel.
    import glob
    stale = []
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[3-9]_traffic*.json"))):
        try:
            tj = json.load(open(path))
        except (OSError, ValueError):
            continue
        if tuple(tj.get("shape", ())) != (Cc, H, W):
            continue
        row = next((r for r in rows if r["row"] == tj.get("row", "k2s")), None)
        if row is None:
            continue
        if tj.get("src_sha256") != kernel_sources_sha(tj.get("sources", [])):
            stale.append(os.path.basename(path))
            continue
        row["traffic"] = float(tj["hbm_bytes_per_launch"])
        row["traffic_over_algorithmic"] = round(row["traffic"] / row["bytes_per_launch"], 4)
        row["traffic_source"] = tj["source"] + " [" + tj["kernel"] + "]"
    # the DOMINANT kernel of the family = the row with the most time per step (launches per step x average launch): the top-level
    # object describes THAT kernel against its own roof; the flop-weighted family figure of earlier rounds stays under `family`
    dom = max(rows, key=lambda r: r["per_step"] * r["avg_launch_us"])
    pipe = None
    if Cc > 16:
        # these layers run on the 16-bit matrix pipe, six bf16 products per f32 product: the hardware roof of THAT instruction mix in
        # f32-equivalent flops is the dense bf16 peak / 6; `peak` / `frac` stay priced against the fp32 MFMA peak of the arithmetic type
        pipe = {"instruction": "v_mfma_f32_16x16x32_bf16, 6 products per f32 product (bf16x6)", "peak": round(PEAK_BF16_MFMA_TFLOPS / 6, 1),
                "frac": round(ach / (PEAK_BF16_MFMA_TFLOPS / 6), 4), "unit": "TFLOP/s (f32-equivalent)"}
    if dom["bound"] == "mfma" and Cc > 16:
        # priced against the roof of the pipe the kernel actually runs on (bf16x6: dense bf16 peak / 6 in f32-equivalent flops); the
        # figure against the fp32 MFMA peak of the arithmetic type -- which round 4 put in `frac` -- rides along as `frac_vs_fp32_mfma`
        top = {"bound": "mfma", "achieved": dom["achieved"], "peak": round(PEAK_BF16_MFMA_TFLOPS / 6, 1), "unit": "TFLOP/s (f32-equivalent, bf16x6 split products)",
               "frac": round(dom["achieved"] / (PEAK_BF16_MFMA_TFLOPS / 6), 4), "frac_vs_fp32_mfma": dom["frac"], "peak_fp32_mfma": PEAK_FP32_MFMA_TFLOPS}
    elif dom["bound"] == "mfma":
        top = {"bound": "mfma", "achieved": dom["achieved"], "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": dom["frac"]}
    else:
        top = {"bound": "hbm", "achieved": dom["algorithmic_GB_per_s"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(dom["algorithmic_GB_per_s"] / PEAK_HBM_GBS, 4)}
    top.update({"kernel": f"{dom['kernel']} ({Cc}->{Cc} 3x3 @{H}x{W}); dominant = most time per step of the final-stage conv family ({dom['per_step']} x {dom['avg_launch_us']} us)",
                "traffic": dom.get("traffic"), "traffic_unit": "bytes/launch",
                "traffic_source": dom.get("traffic_source") or ("no valid PMC profile of this row" + (f" (stale, measured on other kernel sources: {', '.join(stale)})" if stale else "") + "; run tools/pmc_traffic.py"),
                "avg_launch_us": dom["avg_launch_us"], "flops_per_launch": dom["flops_per_launch"], "bytes_per_launch": dom["bytes_per_launch"],
                "family": {"what": f"final-stage conv family of the step ({Cc}->{Cc} 3x3 @{H}x{W}): flop-weighted over the {nl} launches of a step listed under `kernels`",
                           "achieved": round(ach, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_FP32_MFMA_TFLOPS, 4),
                           "frac_of_per_kernel_roof": round(troof / tt, 4), "avg_launch_us": round(tt / nl * 1e6, 2), "split_pipe": pipe,
                           "slowest": {"kernel": slow["kernel"], "achieved": slow["achieved"], "frac": slow["frac"]}},
                "kernels": rows})
    return top


def kernel_sources_sha(files):
    """SHA-256 over the named kernel sources (relative to boosting_nerv_amd/csrc), the stamp of a PMC traffic profile."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(files):
        try:
            h.update(open(os.path.join(ROOT, "boosting_nerv_amd", "csrc", f), "rb").read())
        except OSError:
            return None
    return h.hexdigest() if files else None


def cpu_model_string():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, model_cpu_sd, frames, norm_idxs, budget_s=30.0, max_steps=20):
    """SURVEY 8(d) protocol: the oracle restatement of the SAME train step on this box's host cores for a bounded sample.  The thread
    count is MEASURED, not assumed (the MKLDNN convolutions of these shapes do not scale to every core of a 2-socket host): after one
    untimed step, one untimed + two timed steps at each of 16 / 32 / 64 threads (as many as the box has), then the remaining budget at
    the best setting; the reported value is the best setting's rate over all its timed steps, `cores` its thread count, `sweep` the
    per-setting rates.  Models whose step takes longer than a tenth of the budget (the 1080p configs: 10-25 s per step) sweep with ONE
    timed step per setting (round 4 skipped their sweep and quoted the 64-thread figure, which the C1 sweep shows to be 2.3x too slow)
    -- the sample string says what was run."""
    from oracle import cpu_ref
    hw = os.cpu_count() or 1
    sd = {k: v.clone().float().requires_grad_(True) for k, v in model_cpu_sd.items()}
    adan = cpu_ref.AdanState(list(sd.values()), lr=args.lr)
    kind = args.model
    k = [0]

    def one():
        i = k[0] % frames.shape[0]
        k[0] += 1
        t = time.time()
        cpu_ref.train_step(kind, sd, adan, frames[i:i + 1], norm_idxs[i:i + 1], args.loss)
        return time.time() - t

    t_all = time.time()
    torch.set_num_threads(min(hw, 64))
    one()                                                    # untimed: lazy initialisation, page faults of the first step
    t_probe = one()
    sweep, best = {}, min(hw, 64)
    slow = t_probe * 10 > budget_s                           # the 1080p configs (10-25 s per step): ONE timed step per setting, no untimed one
    sweep_t = {}
    for nt in sorted({min(hw, c) for c in (16, 32, 64)}):
        torch.set_num_threads(nt)
        if not slow:
            one()
        ts = [one()] if slow else [one(), one()]
        sweep[nt] = round(len(ts) / sum(ts), 4)
        sweep_t[nt] = (len(ts), sum(ts))
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    n, t0 = 0, time.time()
    step_ts = []
    if slow:
        # the best setting's sweep step counts; more steps only while the whole baseline stays inside 4 x the budget
        n, dt = sweep_t[best]
        while n < max_steps and (time.time() - t_all) + dt / n < 4 * budget_s:
            dt += one()
            n += 1
    else:
        while n < max_steps and (n == 0 or (time.time() - t_all) < budget_s + 15.0) and (n == 0 or time.time() - t0 < budget_s):
            step_ts.append(one())
            n += 1
        dt = time.time() - t0
    spread = None
    if step_ts:
        st = sorted(step_ts)
        spread = {"min": round(st[0], 3), "median": round(st[len(st) // 2], 3), "max": round(st[-1], 3)}     # (the mean above is the reported rate; host steps vary with thread placement)
    return {"value": round(n / dt, 4), "unit": "frames/s", "cores": best, "host_cores": hw, "kind": "port", "cpu": cpu_model_string(),
            "sweep_frames_per_s_by_threads": sweep or None, "step_seconds": spread,
            "sample": f"{n} timed full train steps (fwd + {args.loss} + bwd + Adan) of the same model / frame size at the best of the swept thread counts "
                      f"({best} threads; sweep: {'1 timed step per setting, a step takes more than a tenth of the budget' if slow else '1 untimed + 2 timed steps per setting'}), "
                      f"oracle/cpu_ref.py on torch CPU fp32, timed budget {budget_s:.0f} s"}


def parity_leg(args, model, opt, step_fn, frames, norm, takes_image, s0, n_iter, set_lr, K=3, budget_s=60.0):
    """Checker leg (like cpu_baseline: the oracle is only the yardstick here).  From the state the timed steps left behind -- parameters
    AND optimizer state -- K further train steps on the HIP path and on oracle/cpu_ref.py (same frames, same learning rates), compared
    step by step: max |image difference| of the forward at the step's parameters, relative loss difference, train-PSNR difference in
    dB.  north_star's gate: PSNR within +-0.02 dB, per-pixel fp32 rtol 1e-3."""
    from oracle import cpu_ref
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    named = dict(model.named_parameters())
    sd = {k: v.detach().cpu().clone().float().requires_grad_(True) for k, v in model.state_dict().items()}
    adan = cpu_ref.AdanState(list(sd.values()), lr=args.lr)
    for i, k in enumerate(sd):
        st = opt.state.get(named.get(k), {})
        if "exp_avg" in st:
            adan.m[i], adan.n[i], adan.d[i] = st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["exp_avg_diff"].cpu().clone()
            adan.prev[i] = -st["neg_pre_grad"].cpu()
    adan.step_n = int(opt.param_groups[0].get("step", 0))
    rows, t0 = [], time.time()
    for j in range(K):
        if j > 0 and time.time() - t0 > budget_s:
            break
        s = s0 + j
        i = s % n_iter
        set_lr(s, i)
        adan.lr = float(opt.param_groups[0]["lr"])
        with torch.no_grad():
            model.eval()
            img_h = model(frames[i:i + 1] if takes_image else norm[i:i + 1], norm_idx=norm[i:i + 1])[0].float().cpu()
            model.train()
        loss_h, psnr_h = step_fn(i)
        loss_h, psnr_h = float(loss_h.item()), float(psnr_h.mean().item())
        loss_c, psnr_c, img_c = cpu_ref.train_step(args.model, sd, adan, frames[i:i + 1].cpu(), norm[i:i + 1].cpu(), args.loss)
        rows.append({"max_abs_img": float((img_h - img_c).abs().max()), "max_rel_img": float(((img_h - img_c).abs() / (1e-5 / 1e-3 + img_c.abs())).max()),
                     "rel_loss": abs(loss_h - float(loss_c)) / max(abs(float(loss_c)), 1e-12), "dpsnr_db": psnr_h - float(psnr_c.mean())})
    worst = {"max_abs_img": max(r["max_abs_img"] for r in rows), "rel_loss": max(r["rel_loss"] for r in rows), "dpsnr_db": max((r["dpsnr_db"] for r in rows), key=abs)}
    ok = all(r["max_rel_img"] <= 1e-3 for r in rows) and abs(worst["dpsnr_db"]) <= 0.02
    return {"max_abs_img": float(f"{worst['max_abs_img']:.3e}"), "rel_loss": float(f"{worst['rel_loss']:.3e}"), "dpsnr_db": round(worst["dpsnr_db"], 5),
            "steps": len(rows), "per_step": [{k: float(f"{v:.3e}") for k, v in r.items()} for r in rows],
            "gate": "every pixel |hip - oracle| <= 1e-5 + 1e-3 |oracle| and |dPSNR| <= 0.02 dB", "within_gate": bool(ok),
            "what": f"{len(rows)} further train steps after the timed region, HIP path vs oracle/cpu_ref.py (CPU fp32) from the SAME parameters and Adan state, "
                    f"same frames and learning rates, {args.loss}"}


@torch.no_grad()
def eval_psnr(model, frames, norm, takes_image, n_eval=8):
    """pred_seen_psnr of evaluate() (train_nerv_all.py:527-550 of the reference) on the first frames of this rank's shard, fp32 model,
    after the timed steps: mean over frames of -10 log10(mse + 1e-9)."""
    from boosting_nerv_amd import ops
    model.eval()
    vals = []
    for i in range(min(n_eval, frames.shape[0])):
        inp = frames[i:i + 1] if takes_image else norm[i:i + 1]
        img = model(inp, norm_idx=norm[i:i + 1])[0]
        vals.append(ops.psnr(img, frames[i:i + 1]))
    model.train()
    return torch.cat(vals).mean().item(), len(vals)


def stock_rocm_yardstick(args, model_cpu_sd, frames, norm_idxs, dev, budget_s=10.0, max_steps=20):
    """SURVEY 8(d) second yardstick: the SAME restatement (oracle/cpu_ref.py, plain torch ops) executed on the GPU by stock
    PyTorch-ROCm (MIOpen convs, hipFFT, eager elementwise).  Reported next to the CPU baseline, never as `value`."""
    from oracle import cpu_ref
    sd = {k: v.clone().float().to(dev).requires_grad_(True) for k, v in model_cpu_sd.items()}
    adan = cpu_ref.AdanState(list(sd.values()), lr=args.lr)
    fr, ni = frames.to(dev), norm_idxs.to(dev)
    for _ in range(3):                                      # warm-up (MIOpen solver search happens here)
        cpu_ref.train_step(args.model, sd, adan, fr[0:1], ni[0:1], args.loss)
    torch.cuda.synchronize()
    n, t0 = 0, time.time()
    while n < max_steps and (time.time() - t0) < budget_s:
        i = (n + 1) % fr.shape[0]
        cpu_ref.train_step(args.model, sd, adan, fr[i:i + 1], ni[i:i + 1], args.loss)
        torch.cuda.synchronize()
        n += 1
    dt = time.time() - t0
    return {"value": round(n / dt, 3), "unit": "frames/s", "kind": "oracle restatement on stock PyTorch-ROCm ops (MIOpen/hipFFT), same GPU",
            "sample": f"{n} full train steps after 3 warm-up"}


def stock_rocm_child(config, budget_s):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--config", config, "--stock_only"]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=budget_s)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            return json.loads(lines[-1])
        return {"value": None, "error": (r.stderr or r.stdout)[-200:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "note": f"not finished within the {budget_s:.0f} s budget (MIOpen solver search on a fresh box); --stock_rocm allows 240 s", "waited_s": round(time.time() - t0, 1)}
    except Exception as e:       # the yardstick must never take the bench line down
        return {"value": None, "error": f"{type(e).__name__}: {e}"[:200]}


def other_config_child(config, steps, budget_s):
    """`python bench.py --config <c> --brief` in a child process (its own HIP context and memory pool): the captured step of another
    BASELINE config timed over `steps` replays, plus the dominant final-stage kernel's roofline row.  Never takes the C1 line down."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--config", config, "--brief", "--steps", str(steps), "--warmup", "5"]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=budget_s)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            o = json.loads(lines[-1])
            o["wall_s"] = round(time.time() - t0, 1)
            return o
        return {"value": None, "error": (r.stderr or r.stdout)[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "note": f"not finished within the {budget_s:.0f} s budget", "waited_s": round(time.time() - t0, 1)}
    except Exception as e:       # noqa: BLE001
        return {"value": None, "error": f"{type(e).__name__}: {e}"[:200]}


def device_settle(dev):
    """Bring the device to its steady power / clock state before the timed region WITHOUT touching the model: ~300 ms of fp32 matrix
    work on scratch tensors.  Measured on MI355X (tools/ktransient.py, profiles/r06_transient.md): after the host-bound eager steps and the
    graph capture (GPU idle for ~60 ms) the first ~16 replays of the captured step run 1.65 -> 1.46 ms, a smooth ramp of the matrix
    pipe's power state -- 80 ms of matmul before them removes it, 80 ms of copies or of sleeping does not.  A W = 5 / K = 20 invocation
    would otherwise time exactly that ramp (1.50 ms) instead of the rate every later step of a 39 600-step schedule runs at (1.455 ms).
    The timed region is unchanged: exactly K full train steps between two synchronisations.  BNERV_BENCH_SETTLE_MS=0 switches it off."""
    ms = float(os.environ.get("BNERV_BENCH_SETTLE_MS", "300"))
    if ms <= 0:
        return 0.0
    n_ = int(os.environ.get("BNERV_BENCH_SETTLE_N", "4096"))
    a_ = torch.randn(n_, n_, device=dev)
    b_ = torch.randn(n_, n_, device=dev)
    torch.mm(a_, b_)                                     # (the first call loads the BLAS library and picks a kernel: host time, no load)
    torch.cuda.synchronize()
    t0 = time.time()
    while (time.time() - t0) * 1e3 < ms:
        for _ in range(8 * max(1, (4096 // n_) ** 2)):
            torch.mm(a_, b_)
        torch.cuda.synchronize()
    return round((time.time() - t0) * 1e3, 1)


def last_stage_channels(model):
    """Channel count of the decoder's last stage = input channels of the head conv."""
    m = model
    for name in ("head_layer", "head_layers"):
        hl = getattr(m, name, None)
        if hl is None:
            continue
        if isinstance(hl, torch.nn.ModuleList):
            hl = [x for x in hl if x is not None][-1]
        conv = hl if hasattr(hl, "weight") else next(x for x in hl.modules() if hasattr(x, "weight") and x.weight.dim() == 4)
        return int(conv.weight.shape[1])
    raise RuntimeError("no head layer found")


def dump_outputs(out_dir, step, model, budget_bytes=60_000_000):
    """--dump-outputs: what the last timed step handed its caller -- loss, per-sample PSNR (bpp for the compression step) and the
    updated model tensors -- as float32 .npy files.  Tensors are taken smallest first; one larger than its even share of what is
    left of the budget is written as a fixed seeded sample of its flattened elements (same indices on every run)."""
    import numpy as np
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    arrays = {"loss": step.loss_out, "psnr": step.psnr_out}
    if getattr(step, "bpp_out", None) is not None:
        arrays["bpp"] = step.bpp_out
    for k, v in model.state_dict().items():
        if torch.is_floating_point(v):
            arrays["param." + k] = v
    os.makedirs(out_dir, exist_ok=True)
    left, items = budget_bytes, sorted(arrays.items(), key=lambda kv: (kv[1].numel(), kv[0]))
    for j, (name, t) in enumerate(items):
        a = t.detach().float().cpu().numpy()
        share = left // (len(items) - j)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=max(share // 4, 1), replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32, copy=False))
        left -= a.nbytes
    return len(items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="c1", choices=sorted(RECIPES))
    ap.add_argument("--no_graph", action="store_true")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--steps_only", action="store_true", help="profiling aid: time the steps and print a short line (no kernel micro-benchmark, eval, CPU baseline)")
    ap.add_argument("--brief", action="store_true", help="child mode of the C1 line's `other_configs`: time the steps, add the dominant final-stage kernel's roofline row, print one short JSON object")
    ap.add_argument("--stock_only", action="store_true", help="child mode of the stock-ops yardstick: print its JSON object and exit")
    ap.add_argument("--stock_rocm", action="store_true", help="with --full: give the stock PyTorch-ROCm yardstick 240 s instead of 75 s (slow first run)")
    ap.add_argument("--full", action="store_true", help="besides the headline: kernel roofline, parity, host-frames rate, other configs, eval PSNR, "
                                                        "CPU baseline and stock-ops yardstick (off: set up, warm up, time the steps, print the line)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (loss, PSNR, updated model tensors) to DIR/<name>.npy, float32, <= 64 MB")
    a = ap.parse_args()

    if a.stock_only:
        from boosting_nerv_amd.synth import SyntheticVideo
        args, model = build(a.config)
        r = RECIPES[a.config]
        vid = SyntheticVideo(r["n"], r["h"], r["w"])
        fcpu = torch.stack([vid.frame(i) for i in range(4)])
        ncpu = torch.tensor([(i + 1) / r["n"] for i in range(4)], dtype=torch.float64)
        torch.backends.cudnn.benchmark = False
        print(json.dumps(stock_rocm_yardstick(args, {k: v.clone() for k, v in model.state_dict().items()}, fcpu, ncpu, torch.device("cuda", 0))), flush=True)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: launch ourselves one rank per GPU (what the reference does with mp.spawn from one command,
        # train_nerv_all.py:139-148) -- the same torch.distributed.run line the driver uses, on a free local port
        import socket
        share_ = os.environ.get("BNERV_BENCH_SHARE_GPU", "0") == "1"
        if not share_ and torch.cuda.device_count() < a.gpus:
            raise SystemExit(f"bench.py --gpus {a.gpus}: only {torch.cuda.device_count()} GPU(s) visible on this node")
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        import subprocess
        raise SystemExit(subprocess.call(cmd))      # (a fresh child process: this one may already hold the HIP runtime)
    if world != a.gpus:
        raise SystemExit(f"bench.py --gpus {a.gpus} started with WORLD_SIZE={world}: launch one rank per GPU (or run plain `python bench.py --gpus N`)")
    assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback for the product path)"
    # Test hook (never set by the driver): BNERV_BENCH_SHARE_GPU=1 runs all ranks of an N > 1 launch on device 0 over gloo, so the
    # multi-GPU code path of this script can be smoke-tested on a 1-GPU box.  The numbers of such a run mean nothing.
    share = os.environ.get("BNERV_BENCH_SHARE_GPU", "0") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group(backend="gloo" if share else "nccl", init_method="env://", world_size=world, rank=rank)
    # Test hook (never set by the driver): BNERV_BENCH_FORCE_BUCKET=1 runs the N = 1 bench through the multi-GPU step (bucket gather ->
    # RCCL all-reduce on a 1-rank group -> scatter, captured in the step graph) -- the single-GPU cost of that path, with one or two
    # bucket segments (BNERV_DP_BUCKETS), is the only part of the N > 1 step a 1-GPU box can measure.
    force_bucket = world == 1 and os.environ.get("BNERV_BENCH_FORCE_BUCKET", "0") == "1"
    if force_bucket:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29655")
        dist.init_process_group(backend="nccl", rank=0, world_size=1)

    from boosting_nerv_amd.dp import shard_indices
    from boosting_nerv_amd.engine import TrainStep
    from boosting_nerv_amd.hnerv_utils import adjust_lr
    from boosting_nerv_amd.optimizer import Adan
    from boosting_nerv_amd.synth import SyntheticVideo

    args, model = build(a.config)
    sd_cpu = {k: v.clone() for k, v in model.state_dict().items()}
    n_params = sum(p.numel() for p in model.parameters())
    model = model.to(dev)
    opt = Adan(model.parameters(), lr=args.lr)
    r = RECIPES[a.config]
    vid = SyntheticVideo(r["n"], r["h"], r["w"])
    my_idx = shard_indices(r["n"], rank, world, seed=0)            # DistributedSampler's shard of the frame set (all frames at N=1)
    keep = my_idx[:min(len(my_idx), 48 if r["h"] > 720 else 132)]
    frames = torch.stack([vid.frame(i, device=dev) for i in keep])  # resident in HBM before the timed region
    norm = torch.tensor([(i + 1) / r["n"] for i in keep], dtype=torch.float64, device=dev)
    takes_image = "HNeRV" in args.model
    per_gpu_batch = 1
    step = TrainStep(model, opt, args.loss, takes_image, (per_gpu_batch, 3, r["h"], r["w"]), dev, use_graph=not a.no_graph,
                     warmup_eager=3, world_size=world, force_bucket=force_bucket)
    args.epochs = 300
    n_iter = len(keep)

    if a.config == "c5":                                       # compression step (train_nerv_compression.py:354-367)
        from boosting_nerv_amd import ops
        from boosting_nerv_amd.hnerv_utils import loss_fn
        from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
        em = DiffEntropyModel("gaussian")
        model.init_data()
        model.train()
        final_size, n_full = r["h"] * r["w"], r["n"]
        target_bpp = args.target_bit * (sum(p.numel() for p in model.parameters()) / 1e6) * 1e6 / final_size / n_full

        from boosting_nerv_amd.engine import CompressionStep
        args.final_size, args.full_data_length, args.target_bpp = final_size, n_full, target_bpp
        step = CompressionStep(model, opt, em, args, (per_gpu_batch, 3, r["h"], r["w"]), dev, use_graph=not a.no_graph, warmup_eager=3)

    # the shard is resident in HBM: the step picks its frame by index (one 32-byte host -> device record per step, TrainStep.bind_clip)
    by_index = a.config != "c5" and os.environ.get("BNERV_BENCH_COPY_FRAMES", "0") != "1"
    if by_index:
        step.bind_clip(frames, norm)

    def run(k0, k):
        for s in range(k0, k0 + k):
            i = s % n_iter
            adjust_lr(opt, (s / n_iter) / args.epochs, i, args)
            if by_index:
                step.step_frame(i)
            else:
                step(frames[i:i + 1], norm[i:i + 1])

    # ---- N > 1: make the run self-diagnosing (nothing here is inside the timed region) -----------------------------------------------
    # (a) the flat bucket's all-reduce alone, timed on its own (bucket-size fp32 tensor, 20 repetitions after 3 warm-ups);
    # (b) both bucket layouts of the step -- one segment, and two segments with the early one overlapped with the stem's backward
    #      -- 20 steps each after their own eager warm-up + capture; the faster one (max over ranks, so every rank
    #     picks the same) runs the W warm-up and the K timed steps.  BNERV_DP_BUCKETS pins the layout and skips the probe.
    dp_diag = None
    if (world > 1 or force_bucket) and a.config != "c5":
        def timed_steps(stp, k0, k):
            for s_ in range(k0, k0 + k):
                i_ = s_ % n_iter
                adjust_lr(opt, (s_ / n_iter) / args.epochs, i_, args)
                stp.step_frame(i_) if by_index else stp(frames[i_:i_ + 1], norm[i_:i_ + 1])

        def probe(stp, k=20):
            timed_steps(stp, 0, 6)                              # 3 eager + capture + 2 replays
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            t_ = time.time()
            timed_steps(stp, 6, k)
            torch.cuda.synchronize()
            tt_ = torch.tensor([(time.time() - t_) / k * 1e3], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
            return round(tt_.item(), 4)

        buf = torch.zeros(n_params, dtype=torch.float32, device=dev)
        for _ in range(3):
            dist.all_reduce(buf)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t_ = time.time()
        for _ in range(20):
            dist.all_reduce(buf)
        torch.cuda.synchronize()
        ar = torch.tensor([(time.time() - t_) / 20 * 1e6], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(ar, op=dist.ReduceOp.MAX)
        dp_diag = {"allreduce_us": round(ar.item(), 1), "allreduce_bytes": n_params * 4,
                   "allreduce_what": "one all_reduce(SUM) of a bucket-size fp32 tensor on this process group, mean of 20 back-to-back calls after 3 warm-ups, host-synchronised, max over ranks"}
        pinned = os.environ.get("BNERV_DP_BUCKETS")

        def restore_fresh():
            """The probes train for real (2 x 26 steps): put parameters and Adan state back to the seeded initial state IN PLACE (the
            captured graphs keep their addresses), so the warm-up and the timed steps -- and the eval PSNR / loss quoted after them --
            start from random init exactly as the N = 1 line does (step count 0: the next step is Adan's first again)."""
            with torch.no_grad():
                for p_, p0_ in zip(model.parameters(), params0):
                    p_.copy_(p0_)
                for st_ in opt.state.values():
                    for v_ in st_.values():
                        if torch.is_tensor(v_):
                            v_.zero_()
            for g_ in opt.param_groups:
                g_["step"] = 0

        if pinned is None and hasattr(model, "dp_late_parameters"):
            params0 = [p_.detach().clone() for p_ in model.parameters()]
            probe_ms = {"1": probe(step)}
            restore_fresh()
            model.dp_hook = None
            step2 = TrainStep(model, opt, args.loss, takes_image, (per_gpu_batch, 3, r["h"], r["w"]), dev, use_graph=not a.no_graph,
                              warmup_eager=3, world_size=world, force_bucket=force_bucket, dp_buckets=2)
            if by_index:
                step2.bind_clip(frames, norm)
            probe_ms["2"] = probe(step2)
            restore_fresh()
            del params0
            if probe_ms["2"] < probe_ms["1"]:
                step = step2
            else:
                model.dp_hook = None                            # (step 1's graph was captured without the hook; eager steps must not call step 2's)
                del step2
            dp_diag["probe_ms_per_step"] = probe_ms
        dp_diag["dp_buckets"] = 2 if (step.bucket is not None and step.bucket.two) else 1

    run(0, max(a.warmup, 5))
    settle_ms = device_settle(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    run(max(a.warmup, 5), a.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.time() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = tt.item()
    loss, psnr = step.loss_out.item(), step.psnr_out.mean().item()
    replicas_in_sync = None
    if world > 1:
        # every rank started from the same seeded parameters and applied the same averaged gradients: the replicas must hold the SAME
        # bits after the timed steps -- a collective that was captured but did not exchange, or exchanged out of order, shows up here
        ck = torch.stack([p.detach().double().sum() for p in model.parameters()] + [p.detach().double().abs().sum() for p in model.parameters()])
        lo, hi = ck.clone(), ck.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_in_sync = bool(torch.equal(lo, hi))
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, step, model)      # (before anything below trains further: parity, host frames)
    if rank == 0 and a.steps_only:
        print(json.dumps({"metric": "train frames/sec", "value": round(a.steps * per_gpu_batch * world / dt, 2), "ms_per_step": round(dt / a.steps * 1e3, 4), "steps_only": True, "settle_ms": settle_ms}), flush=True)
    elif rank == 0 and a.brief:
        rf = step_kernel_roofline(dev, last_stage_channels(model), r["h"], r["w"], reps=8 if r["h"] > 720 else 20)
        fl, by = STEP_WORK[a.config]
        t_step = dt / a.steps
        o = {"config": a.config, "baseline_config": {"c1": "configs[1]", "c3": "configs[2]", "c4": "configs[3]", "c5": "configs[4]"}[a.config], "workload": r["name"] + f" {r['h']}x{r['w']}",
             "value": round(a.steps / dt, 2), "unit": "frames/s", "ms_per_step": round(t_step * 1e3, 4), "steps": a.steps, "last_loss": round(loss, 6), "last_train_psnr_db": round(psnr, 4),
             "step_frac_of_fp32_roof": round(max(fl / (PEAK_FP32_MFMA_TFLOPS * 1e12), by / (PEAK_HBM_GBS * 1e9)) / t_step, 4),
             "dominant_kernel": {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "frac_vs_fp32_mfma", "avg_launch_us")}}
        dom = max(rf["kernels"], key=lambda q: q["per_step"] * q["avg_launch_us"])
        if "frac_of_split_pipe" in dom:
            o["dominant_kernel"]["frac_of_split_pipe"] = dom["frac_of_split_pipe"]
            o["step_frac_of_split_pipe_roof"] = round(fl / (PEAK_BF16_MFMA_TFLOPS / 6 * 1e12) / t_step, 4)
        print(json.dumps(o), flush=True)
    elif rank == 0:
        frames_total = a.steps * per_gpu_batch * world
        out = {"metric": "train frames/sec", "value": round(frames_total / dt, 2), "unit": "frames/s", "n_gpus": world, "steps": a.steps,
               "warmup": max(a.warmup, 5), "ms_per_step": round(dt / a.steps * 1e3, 4), "higher_is_better": True,
               # per step every GPU trains ONE frame of its shard (the reference's `-b N -d`): per-GPU work per step is fixed -> "weak"
               # by the contract's definition; the CLIP is fixed (132 / 600 frames sharded like DistributedSampler), so value =
               # frames/s of one video and value(N) / value(1) is north_star's strong-scaling factor of an epoch
               "scaling": "weak",
               "vs_baseline": None, "dtype": "fp32", "data": "synthetic",
               # tensors, accumulators and every elementwise op are fp32.  The 3x3 convs with more than 16 input or output channels
               # (none in C1 above 45x80; the 22..95-channel stages of C3 / C4) form their products on the 16-bit matrix pipe from
               # THREE bf16 pieces per fp32 operand and six partial products accumulated in fp32 -- measured error 7.9e-8 * sum|a b|,
               # below the 1.3e-7 of the f32 MFMA's own k-ordered chain (profiles/r02_split_kernels.md); BNERV_SPLIT_WIDE=off keeps
               # them on v_mfma_f32_16x16x4_f32
               "arithmetic": "fp32 storage / accumulation; layers with more than 16 channels (convs, data and weight gradients): exact 3-piece bf16 split products (bf16x6, error below the f32 MFMA's own) on v_mfma_f32_16x16x32_bf16"
               if a.config != "c1" else "fp32 (v_mfma_f32_16x16x4_f32) for the 12-channel layers; the 12->48 up-convs and the 30-channel stage: exact bf16x6 split products on v_mfma_f32_16x16x32_bf16",
               "config": {"workload": f"{r['name']} ({n_params} params, fc_dim {args.fc_dim}) train step on a synthetic "
                                      f"{'Bunny' if a.config == 'c1' else 'UVG'}-shaped clip {r['n']}x3x{r['h']}x{r['w']}: "
                                      f"{'quantise + rate term (CEM) + ' if a.config == 'c5' else ''}decoder fwd + {args.loss} + bwd + "
                                      f"{'flat-bucket RCCL all-reduce + ' if world > 1 else ''}fused Adan; frames resident in HBM",
                          "baseline_config": {"c1": "configs[1]", "c3": "configs[2]", "c4": "configs[3]", "c5": "configs[4]"}[a.config], "global_batch": per_gpu_batch * world,
                          "per_gpu_batch": per_gpu_batch, "parallelism": f"dp{world}", "hipgraph": not a.no_graph,
                          "rccl_ranks": (dist.get_world_size() if (world > 1 and dist.get_backend() == "nccl") else 0),
                          "collective_in_graph": bool(getattr(step, "collective_in_graph", False)), "replicas_in_sync": replicas_in_sync,
                          "dp_mode": (None if step.bucket is None else "eager" if step.graph_a is None else "in_graph" if step.collective_in_graph else "two_graph"),
                          "dp_buckets": (None if dp_diag is None else dp_diag["dp_buckets"]),
                          "last_loss": round(loss, 6), "last_train_psnr_db": round(psnr, 4),
                          "settle": f"{settle_ms} ms of fp32 matmul on scratch tensors between the warm-up steps and the timed region (device power-state ramp, bench.device_settle; no model work)"}}
        if dp_diag is not None:
            out["dp"] = dp_diag
            out["allreduce_us"] = dp_diag["allreduce_us"]
        if world > 1 and not replicas_in_sync:
            out["error"] = "replicas diverged: the ranks do not hold the same parameter bits after the timed steps (the gradient exchange did not run, or ran out of order)"
        # --full: everything past the headline -- kernel roofline, parity, host frames, recorded recipe, other configs, eval PSNR, baselines
        if a.full:
            out["roofline"] = step_kernel_roofline(dev, last_stage_channels(model), r["h"], r["w"], reps=20 if r["h"] <= 720 else 8)
        fl, by = STEP_WORK[a.config]
        t_step = dt / a.steps / per_gpu_batch                                   # seconds per trained frame on one GPU
        t_roof = max(fl / (PEAK_FP32_MFMA_TFLOPS * 1e12), by / (PEAK_HBM_GBS * 1e9))
        out["step_roofline"] = {"flops_per_frame": fl, "bytes_per_frame": by, "t_roof_ms": round(t_roof * 1e3, 4), "bound": "mfma" if fl / (PEAK_FP32_MFMA_TFLOPS * 1e12) >= by / (PEAK_HBM_GBS * 1e9) else "hbm",
                                "achieved_TFLOPs": round(fl / t_step / 1e12, 2), "achieved_GBs": round(by / t_step / 1e9, 1), "frac_of_t_roof": round(t_roof / t_step, 4),
                                "note": "algorithmic conv+dense work of one trained frame (BASELINE.md section 3) against the whole measured step, loss / optimizer / launches included"}
        if a.full and world == 1 and not a.no_cpu_baseline and a.config != "c5":
            def set_lr(sg, ig):
                adjust_lr(opt, (sg / n_iter) / args.epochs, ig, args)
            out["parity"] = parity_leg(args, model, opt, (lambda ig: step.step_frame(ig)) if by_index else (lambda ig: step(frames[ig:ig + 1], norm[ig:ig + 1])),
                                       frames, norm, takes_image, max(a.warmup, 5) + a.steps, n_iter, set_lr, K=3 if r["h"] <= 720 else 2)
        if a.full and world == 1 and not a.no_cpu_baseline and a.config != "c5":
            # the end-to-end rate with the frame crossing PCIe every step (pinned host clip -> device copy -> step), next to
            # `value` (frames resident in HBM), never as `value`
            n_h = 40
            host_clip = frames[:min(8, frames.shape[0])].cpu().pin_memory()
            host_norm = norm[:host_clip.shape[0]].cpu().pin_memory()
            for s_ in range(3):
                step(host_clip[s_ % host_clip.shape[0]:s_ % host_clip.shape[0] + 1].to(dev, non_blocking=True), host_norm[s_ % host_clip.shape[0]:s_ % host_clip.shape[0] + 1].to(dev, non_blocking=True))
            torch.cuda.synchronize()
            t_h = time.time()
            for s_ in range(n_h):
                j = s_ % host_clip.shape[0]
                step(host_clip[j:j + 1].to(dev, non_blocking=True), host_norm[j:j + 1].to(dev, non_blocking=True))
            torch.cuda.synchronize()
            t_h = time.time() - t_h
            out["host_frames"] = {"value": round(n_h / t_h, 2), "unit": "frames/s", "ms_per_step": round(t_h / n_h * 1e3, 4),
                                  "what": f"{n_h} steps with the frame copied from pinned host memory each step ({frames[0].numel() * 4 / 1e6:.1f} MB over PCIe) before the same captured step"}
        if a.full and a.config == "c1":
            # the "eval PSNR" half of BASELINE's metric needs the whole schedule (300 epochs): recorded once per round through the CLI
            # (tools/recipe_record.py -> profiles/rNN_cli_c1_e300.json), quoted here next to the live numbers, never as `value`
            import glob
            rec = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[4-9]_cli_c1_e300.json")))
            if rec:
                try:
                    rj = json.load(open(rec[-1]))
                    out["recipe"] = {k: rj.get(k) for k in ("recipe", "epochs", "frames_trained", "wall_s", "train_wo_eval_s", "end_to_end_frames_per_s", "pred_seen_psnr_db",
                                                             "quant_seen_psnr_db", "bpp", "bit_identical_checkpoints", "dataloader_path", "source")}
                    out["recipe"]["recorded"] = "a committed record of an earlier run of the full schedule on an MI355X (not measured by this invocation)"
                except (OSError, ValueError):
                    pass
        if a.full and a.config == "c1" and world == 1 and not a.no_cpu_baseline and os.environ.get("BNERV_BENCH_OTHER", "1") != "0":
            # BASELINE configs[3] / configs[2] beside the headline: the captured step of each, timed in a child process after this
            # line's timed region (the driver only runs C1; profiles/rNN_bench_c{3,4}.json are the long forms of the same numbers)
            out["other_configs"] = {c_: other_config_child(c_, 10, 150.0) for c_ in ("c4", "c3")}
        if a.full:
            ev, nev = eval_psnr(model, frames, norm, takes_image)
            out["eval_psnr_db"] = round(ev, 3)
            out["config"]["eval"] = f"pred_seen_psnr over the first {nev} frames of the shard after {max(a.warmup, 5) + a.steps + (out['parity']['steps'] if 'parity' in out else 0)} train steps from random init (fp32 model)"
        if a.full and world == 1 and not a.no_cpu_baseline:
            fcpu = torch.stack([vid.frame(i) for i in keep[:4]])
            ncpu = torch.tensor([(i + 1) / r["n"] for i in keep[:4]], dtype=torch.float64)
            out["cpu_baseline"] = cpu_baseline(args, sd_cpu, fcpu, ncpu)
            out["gpu_over_cpu"] = round(out["value"] / max(out["cpu_baseline"]["value"], 1e-9), 1)
            # second yardstick of SURVEY 8(d): the same restatement on stock PyTorch-ROCm ops, in a child process under a time budget
            # (on a fresh box MIOpen may compile / search solvers for ~50 conv shapes: minutes) -- the bench line never waits longer
            out["stock_rocm"] = stock_rocm_child(a.config, budget_s=240.0 if a.stock_rocm else 75.0)
        elif a.full:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if dist.is_available() and dist.is_initialized():      # (also the 1-rank group of BNERV_BENCH_FORCE_BUCKET: a live watchdog thread must not meet the teardown)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
    from boosting_nerv_amd.runtime import hard_exit
    hard_exit(0)        # (the line is printed, the process group destroyed: quiesce torch's autograd worker, then the regular teardown -- runtime.hard_exit)
