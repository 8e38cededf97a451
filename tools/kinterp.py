"""Times of the interpolation file on one MI355X, on the seeded H1-size HNeRV model at 1080p over 17 synthetic frames
(--interpolation --data_split 1_1_2: 9 stored frames, 8 derived):

  (1) train_nerv_all.evaluate() under --embed_inter (frames through the loader, the encoder three times per held-out frame) and under
      --embed_inter_stored (resident clip, the encoder once per stored frame, ops.embed_expand): host clock around the call, ending in a device
      synchronisation, the two alternated, the first call of each (code objects, the loader's frame cache) reported apart;
  (2) the embed_expand launch: bnerv_embed_expand captured 50 times into a graph, replayed, HIP events; and ops.embed_expand as the host
      calls it (validation, plan upload, launch);
  (3) the files: .bnrq under the flag against the all-frames .bnrq of the same model (--interpolation without either flag), sizes and
      codec.Decoder ready times, alternated.

Results go to profiles/interp_file.md by hand.  usage: python tools/kinterp.py [--frames 17] [--rounds 3]   (needs the GPU)"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ("--vid h1 --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --loss L2 --enc_strds 5 3 2 2 2 --enc_dim 64_16 "
          "--dec_strds 5 3 2 2 2 --ks 0_1_5 --reduce 1.2 --lower_width 12 --fc_dim 96 --modelsize 1.5 --crop_list 1080_1920 --resize_list -1 -b 1 -j 0 "
          "--interpolation --data_split 1_1_2 -p 1000")


def setup(flags, n_frames, outf, dev):
    """(model, loader, args) as train_nerv_all.train() has them in front of evaluate(), seeded."""
    import torch
    from boosting_nerv_amd import runtime as rt
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import TransformInput
    args = T.parse_args(f"--data_path synthetic:{n_frames}x1080x1920 {RECIPE} {flags}".split())
    args.outf = outf
    os.makedirs(outf, exist_ok=True)
    torch.manual_seed(1)
    full, loader, _train, resident = T._make_loaders(args, 1)
    args.fc_dim, _ = T.solve_fc_dim(args, args.final_size, args.full_data_length)
    args.metric_names = list(rt.METRIC_NAMES)
    torch.manual_seed(1)
    model = T.build_model(args).to(dev)
    args.transform_func = TransformInput(args)
    args._frames_dev = full.to_device(dev) if resident else None
    return model, loader, args, resident


def timed_eval(model, loader, args):
    import torch
    from boosting_nerv_amd import train_nerv_all as T
    torch.cuda.synchronize()
    t0 = time.time()
    values, _ = T.evaluate(model, loader, None, args)
    torch.cuda.synchronize()
    return time.time() - t0, values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import codec, ops, qstream
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import interp_plan
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        runs = {name: setup(flags, a.frames, os.path.join(tmp, name), dev)
                for name, flags in (("embed_inter", "--embed_inter"), ("embed_inter_stored", "--embed_inter_stored"), ("all_frames", ""))}
        for name, (_, _, args, resident) in runs.items():
            print(f"{name}: clip resident {resident}, {args.full_data_length} frames, held out {len(args.val_ind_list)}", flush=True)
        # (1) evaluation
        times = {"embed_inter": [], "embed_inter_stored": []}
        values = {}
        for _ in range(a.rounds + 1):
            for name in times:
                model, loader, args, _ = runs[name]
                dt, values[name] = timed_eval(model, loader, args)
                times[name].append(dt)
        for name, t in times.items():
            print(f"evaluate() under --{name}: first call {t[0]:.3f} s, then best {min(t[1:]) * 1e3:.1f} ms, worst {max(t[1:]) * 1e3:.1f} ms of {len(t) - 1}", flush=True)
        names = runs["embed_inter"][2].metric_names
        same = all(torch.equal(x, y) for n, x, y in zip(names, values["embed_inter"], values["embed_inter_stored"]) if n.startswith("pred_"))
        print("pred_* of the two evaluations equal: " + str(same) + " | " + ", ".join(f"{n} {float(v):.4f}" for n, v in zip(names, values["embed_inter_stored"])), flush=True)

        # (2) the launch
        stored, plan = interp_plan(a.frames, "1_1_2")
        model, loader, args, _ = runs["embed_inter_stored"]
        table = T._encode_stored(model, loader, args, args._frames_dev)
        S, P = table.shape[0], table[0].numel()
        out = torch.empty((a.frames,) + tuple(table.shape[1:]), device=dev)
        plan_dev = ops._upload(plan, dev)
        lib = L.load()
        launch = lambda: L.check(lib.bnerv_embed_expand(L.stream(), L.ptr(table), L.ptr(plan_dev), L.ptr(out), S, a.frames, P), "bnerv_embed_expand")      # noqa: E731
        launch()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.embed_expand(table, plan))
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            with L.graph_capture(g):
                for _ in range(50):
                    launch()
        best = []
        for _ in range(max(a.rounds, 3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1) / 50 * 1e3)
        host = []
        for _ in range(20):
            torch.cuda.synchronize()
            t0 = time.time()
            ops.embed_expand(table, plan, out)
            torch.cuda.synchronize()
            host.append((time.time() - t0) * 1e6)
        print(f"embed_expand [{S}, {P}] -> [{a.frames}, {P}]: launch {min(best):.2f} us best, {max(best):.2f} worst (graph of 50); ops.embed_expand as the host "
              f"calls it, synchronised: {min(host[1:]):.0f} us best, {float(np.median(host[1:])):.0f} median", flush=True)

        # (3) the files
        blobs = {}
        for name in ("embed_inter_stored", "all_frames"):
            model, loader, args, _ = runs[name]
            args.bitstream = os.path.join(tmp, name + ".bnrq")
            T.evaluate(model, loader, None, args, huffman_coding=True)
            blobs[name] = open(args.bitstream, "rb").read()
            b = codec.info(blobs[name])
            q = qstream.read(blobs[name])
            print(f".bnrq {name}: {b['bytes']} bytes, embedding record {q.records[0].count} symbols (shape {q.settings['embed_shape']}), "
                  f"bits per parameter {args.full_bits_per_param:.4f}, bits per pixel {args.total_bpp:.5f} | {codec.describe_any(b)}", flush=True)
        ready = {k: [] for k in blobs}
        for _ in range(max(a.rounds, 3) + 1):
            for name, blob in blobs.items():
                torch.cuda.synchronize()
                t0 = time.time()
                dec = codec.Decoder(blob, dev, use_graph=False)
                torch.cuda.synchronize()
                ready[name].append(time.time() - t0)
                assert len(dec) == a.frames
                del dec
        for name, t in ready.items():
            print(f"Decoder ready, .bnrq {name}: {min(t[1:]) * 1e3:.1f} ms best, {max(t[1:]) * 1e3:.1f} worst of {len(t) - 1} (first call {t[0] * 1e3:.0f} ms)", flush=True)
        d = codec.Decoder(blobs["embed_inter_stored"], dev, use_graph=False)
        assert d.stored_frames == stored and d.embeds.shape[0] == a.frames
        print(f"the interpolation file stores frames {d.stored_frames}", flush=True)


if __name__ == "__main__":
    main()
