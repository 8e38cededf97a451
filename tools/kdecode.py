"""Decode rates on the HIP path.

    python tools/kdecode.py [c1|c3|c4]            forward-only frames/s of a bench.py decoder: eager, captured, engine.DecodeGraph
    python tools/kdecode.py --bitstream [...]     the bitstream decoder (codec.py), below

--bitstream times, in ONE process:
  (1) bitstream -> model-ready: codec.Decoder(file) -- header, host rANS decode of every record, one upload of the symbols, the
      de-quantisation launches, the raw section, the warm-up forwards and (with the graph) the capture -- host clock, ends in a device
      synchronisation; the first construction of the process (code objects, lazily built tables) is reported apart;
  (2) frames per second of the frame loop, replay -> pinned host uint8 (Decoder.frames_u8(copy=False): forward + packing kernel, the
      device-to-host copy into one of two pinned buffers, one event wait per frame), captured graph and eager launches alternated;
  (3) bnerv_frame_to_u8 against the torch expression it replaces, (x.clamp(0, 1) * 255 + 0.5).to(uint8).permute(0, 2, 3, 1).contiguous(),
      at 720p and 1080p: both captured `reps` times into a graph and replayed (HIP events; a Python-driven launch costs more host time
      than either takes on the GPU), alternated over the rounds; outputs compared first.
Cases: "c1q" -- the C1 model (NeRV_Boost 1.5M, 720x1280) built with the compression recipe's quantiser flags; "c5" -- BASELINE configs[4]
(HNeRV_Boost 3M, 1080x1920, quantised embeddings).  Weights are the seeded initialisation with init_data() scales: the timing does not
depend on what the weights say.
--bitstream --posthoc times the file of the regression path instead (qstream.py) on the C1 model as train_nerv_all builds
it: quant_model -> codec.encode_posthoc, then (1) as above -- here the coded bytes go up as they lie in the file and ONE kernel decodes and
de-quantises them -- and the decode kernel alone under HIP events (ops.HuffDequant.launch, tables already on the device; 20 launches replayed from a graph).
--bitstream --chunked compares the two kinds of CEM file of ONE model (c1q, c5): the version-1 file, whose records the host
rANS-decodes, against the chunked file (rstream.py) repacked from it at runs of 256 and 1024, whose words ONE kernel decodes.  (1) as above
for every file, the kinds alternated in one process, eager and graph; the decode launch alone under HIP events (ops.AnsDequant.launch, tables
already on the device; 50 launches replayed from a graph); every file's size and the chunked overhead in bits per symbol.
--bitstream --wide times the decode kernel of the wide kind (wstream.py) on the seeded c1q model in ONE process: the narrow
model's BNRE file under ops.AnsDequantTables and, the same records with shift 0, under ops.AnsDequantWide; then the model with the scale of
its first (stem) weight quantiser cut so that the record spans about 25 000 values -- which only the wide kind holds -- under
ops.AnsDequantWide; the size of that record against its version-1 message.  Times are per launch and per symbol of a run (a lane decodes
its run's symbols one after the other).
--bitstream --temporal compares the temporal kind (tstream.py) with the wide kind of the same run on the seeded c5 model and
--frames consecutive frames of the 1080p synthetic clip (the files of tools/kencode.py --temporal, coded on the device): codec.Decoder ready
times of both kinds alternated in one process; the three launches of the temporal decoder (ops.AnsDequantWide over the tensor records,
ops.AnsDecodeWide over the embedding records, ops.EmbedChainDequant) and the one launch of the wide decoder, each replayed from a graph; the
temporal file decodes to the parameters, the embeddings and the first and last frame of the version-1 file.

--bitstream --posthoc --sparse times the sparse post-hoc file (zstream.py) against the dense file of the SAME pruned model in
ONE process: the seeded C1 model pruned by global magnitude to --sparsity (default 0.4), quantised once with quant_tensor (the .bnrq file)
and once with quant_tensor_sparse (the .bnrz file); model-ready of both files alternated, eager and graph; then the two decode launches
alone under HIP events (ops.HuffDequant.launch / ops.HuffzDequant.launch, 20 launches replayed from a graph each, alternated over the rounds).
--bitstream --posthoc --temporal times the temporal post-hoc file (pstream.py) against the .bnrq file of the same evaluation on
the seeded H1 model of tools/kencode.py --posthoc over --frames consecutive 1080p frames: codec.Decoder ready times of both kinds alternated in one
process; the launches -- ops.HuffDequant over the whole .bnrq file, then over the tensor section alone, ops.HuffDecodeU8 per bit string,
ops.EmbedChainDequantU8, and the encoder's ops.EmbedDeltaU8 -- each from a graph; and a check that both files decode to the same parameters,
embeddings and first and last frame.

usage: python tools/kdecode.py --bitstream [--posthoc [--sparse [--sparsity S]|--temporal]|--chunked|--wide|--temporal] [--frames 16] [--rounds 3] [--only c1q|c5|pack]   (needs the GPU)"""
import argparse
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUANT_FLAGS = ("--embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale "
               "--quantizer_e scalebeta")


def build(case):
    import torch
    import bench
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd import train_nerv_compression as T5
    if case == "c5":
        return bench.build("c5")
    r = bench.RECIPES["c1"]
    args = T5.build_parser().parse_args(r["flags"].split() + QUANT_FLAGS.split() + ["--data_path", f"synthetic:{r['n']}x{r['h']}x{r['w']}", "--vid", "bench"])
    args.final_size, args.full_data_length, args.outf = r["h"] * r["w"], r["n"], "bench"
    args.fc_dim, _ = T.solve_fc_dim(args, args.final_size, args.full_data_length)
    torch.manual_seed(args.manualSeed)
    return args, T.build_model(args)


def time_graph(fns, reps=50, rounds=5):
    """us per call of every fn in fns on the GPU: `reps` calls of each captured into a graph of its own; the graphs replayed in turn,
    `rounds` times; -> [(best, worst)] per fn."""
    import torch
    from boosting_nerv_amd import _lib as L
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs, out = [], [[] for _ in fns]
    with torch.cuda.stream(side):
        for fn in fns:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with L.graph_capture(g, stream=side):
                for _ in range(reps):
                    fn()
            graphs.append(g)
        torch.cuda.synchronize()
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, g in enumerate(graphs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                out[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    torch.cuda.current_stream().wait_stream(side)
    return [(min(v), max(v)) for v in out]


def run_pack(rounds):
    import torch
    from boosting_nerv_amd import ops
    dev = torch.device("cuda:0")
    slower = False
    for name, (h, w) in (("720p", (720, 1280)), ("1080p", (1080, 1920))):
        x = (torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(1)) * 1.2 - 0.1).to(dev)
        buf = torch.empty(1, h, w, 3, dtype=torch.uint8, device=dev)
        chain = lambda: (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()      # noqa: E731
        assert torch.equal(ops.frame_to_u8(x, out=buf), chain())
        (k_lo, k_hi), (t_lo, t_hi) = time_graph([lambda: ops.frame_to_u8(x, out=buf), chain], rounds=max(rounds, 3))
        nbytes = 15 * h * w
        print(f"pack {name}: bnerv_frame_to_u8 {k_lo:.1f} us (worst {k_hi:.1f}; {nbytes / k_lo / 1e3:.0f} GB/s of its 15 B/pixel) | torch chain {t_lo:.1f} us "
              f"(worst {t_hi:.1f}) | torch / kernel = {t_lo / k_lo:.2f}" + ("   ** the kernel is SLOWER **" if k_lo > t_lo else ""), flush=True)
        slower = slower or k_lo > t_lo
    return slower


def run_case(case, n_frames, rounds):
    import torch
    from boosting_nerv_amd import bitstream, codec
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    from boosting_nerv_amd.synth import SyntheticVideo
    dev = torch.device("cuda:0")
    args, model = build(case)
    model = model.to(dev)
    model.init_data()
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    is_hnerv = args.model == "HNeRV_Boost"
    frames = None
    if is_hnerv:
        vid = SyntheticVideo(n_frames, h, w)
        frames = torch.stack([vid.frame(i, device=dev) for i in range(n_frames)])
        with torch.no_grad():
            model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    args.full_data_length = n_frames
    buf = io.BytesIO()
    torch.cuda.synchronize()
    t0 = time.time()
    budget = codec.encode(model, DiffEntropyModel("gaussian"), args, frames, buf)
    torch.cuda.synchronize()
    blob = buf.getvalue()
    n_par = sum(m.weight.numel() + (m.bias.numel() if m.bias is not None else 0) for m in model._quant_modules())
    print(f"{case}: {args.model} {h}x{w}, {n_par} quantised parameters, {n_frames} frames; encode {time.time() - t0:.2f} s; file {codec.describe(budget)}", flush=True)
    del model

    # (1) bitstream -> model-ready
    ready = {}
    for label, use_graph in (("first construction of the process (eager)", False), ("eager", False), ("graph", True), ("eager", False), ("graph", True)):
        t0 = time.time()
        bitstream.read(blob)
        t_read = time.time() - t0
        dec = None                                             # (the previous decoder is released outside the timed window)
        torch.cuda.synchronize()
        t0 = time.time()
        dec = codec.Decoder(blob, dev, use_graph=use_graph)
        torch.cuda.synchronize()
        ready.setdefault(label, []).append(time.time() - t0)
        print(f"{case} model-ready, {label}: {ready[label][-1] * 1e3:.1f} ms (container parse + CRC alone: {t_read * 1e3:.1f} ms)", flush=True)
    dec_g = dec
    dec_e = codec.Decoder(blob, dev, use_graph=False)

    # (2) frame loop: replay -> pinned host u8
    fps = {"graph": [], "eager": []}
    loops = max(1, 64 // n_frames)
    for d in (dec_g, dec_e):                                   # warm-up of both
        for _ in d.frames_u8(copy=False):
            pass
    for r in range(rounds):
        for label, d in (("graph", dec_g), ("eager", dec_e)):
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(loops):
                for _ in d.frames_u8(copy=False):
                    pass
            torch.cuda.synchronize()
            fps[label].append(loops * n_frames / (time.time() - t0))
            print(f"{case} round {r} frame loop, {label}: {fps[label][-1]:.1f} frames/s ({1e3 / fps[label][-1]:.3f} ms/frame)", flush=True)
    for label, v in fps.items():
        print(f"{case} frame loop, {label}: {sum(v) / len(v):.1f} frames/s (min {min(v):.1f}, max {max(v):.1f} over {rounds} rounds of {loops * n_frames} frames)")
    for label, v in ready.items():
        print(f"{case} model-ready, {label}: {min(v) * 1e3:.1f} ms best of {len(v)}")


def run_posthoc(n_frames, rounds):
    import torch
    import bench
    from boosting_nerv_amd import codec, ops, qstream
    from boosting_nerv_amd import train_nerv_all as T
    dev = torch.device("cuda:0")
    args, model = bench.build("c1")
    model = model.to(dev)
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    args.full_data_length, args.final_size = n_frames, h * w
    t0 = time.time()
    _, records = T.quant_model(model, args)
    buf = io.BytesIO()
    budget = codec.encode_posthoc(model, args, records, None, buf)
    blob = buf.getvalue()
    print(f"c1 post hoc: {args.model} {h}x{w}, {budget['n_symbols']} symbols in {budget['n_records']} tensors; quantise + encode {time.time() - t0:.2f} s; "
          f"file {codec.describe_posthoc(budget)}", flush=True)
    del model
    ready = {}
    for label, use_graph in (("first construction of the process (eager)", False), ("eager", False), ("graph", True), ("eager", False), ("graph", True)):
        t0 = time.time()
        qs = qstream.read(blob)
        t_read = time.time() - t0
        dec = None
        torch.cuda.synchronize()
        t0 = time.time()
        dec = codec.Decoder(blob, dev, use_graph=use_graph)
        torch.cuda.synchronize()
        ready.setdefault(label, []).append(time.time() - t0)
        print(f"c1 post hoc model-ready, {label}: {ready[label][-1] * 1e3:.1f} ms (container parse + CRC alone: {t_read * 1e3:.1f} ms)", flush=True)
    for label, v in ready.items():
        print(f"c1 post hoc model-ready, {label}: {min(v) * 1e3:.1f} ms best of {len(v)}")
    # the kernel alone: the same tables, outputs of its own
    items = []
    for r in qs.records:
        tdt = torch.float16 if r.dtype == qstream.F16 else torch.float32
        items.append((torch.empty(r.count, device=dev), torch.from_numpy(r.min).to(dev).to(tdt), torch.from_numpy(r.scale).to(dev).to(tdt), r.red, r.inner, r.run_bits))
    plan = ops.HuffDequant(qs.words, qs.lengths, items)
    plan.launch().check()
    plan.check()
    (best, worst), = time_graph([plan.launch], reps=20, rounds=max(rounds, 3))      # replayed from a graph: a Python-driven launch costs more host time
    plan.check()
    coded = budget["symbol_bits"] / 8
    print(f"c1 post hoc decode kernel: {best:.1f} us best, {worst:.1f} worst per launch ({plan.n_runs} runs, {budget['n_symbols'] / best:.0f} symbols/us, "
          f"{coded / best / 1e3:.2f} GB/s of coded bytes in, {4 * budget['n_symbols'] / best / 1e3:.1f} GB/s of fp32 out)")


def run_posthoc_sparse(n_frames, rounds, sparsity):
    import torch
    import bench
    from boosting_nerv_amd import codec, ops, prune, qstream, zstream
    from boosting_nerv_amd import train_nerv_all as T
    dev = torch.device("cuda:0")
    args, model = bench.build("c1")
    model = model.to(dev)
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    args.full_data_length, args.final_size = n_frames, h * w
    with torch.no_grad():                                      # global magnitude pruning, as prune.Pruner selects (ties aside)
        params = [p for _, p in prune.prunable(model)]
        mags = torch.cat([p.abs().flatten() for p in params])
        tau = mags.kthvalue(max(int(sparsity * mags.numel()), 1)).values
        for p in params:
            p.mul_(p.abs() > tau)
    files = {}
    for kind, flag in (("dense", False), ("sparse", True)):
        args.bitstream_sparse = flag
        _, records = T.quant_model(model, args)
        buf = io.BytesIO()
        budget = codec.encode_posthoc(model, args, records, None, buf)
        files[kind] = (buf.getvalue(), budget)
        print(f"c1 pruned to {sparsity}, {kind} file: {codec.describe_any(budget)}; {budget['symbol_bits'] / budget['n_symbols']:.3f} symbol bits per parameter", flush=True)
    del model
    print(f"c1 pruned to {sparsity}: .bnrz / .bnrq = {files['sparse'][1]['bytes'] / files['dense'][1]['bytes']:.4f}")
    ready = {}
    for r in range(rounds + 1):                                # round 0: the first constructions of the process, reported apart
        for use_graph in (False, True):
            for kind in ("dense", "sparse"):
                torch.cuda.synchronize()
                t0 = time.time()
                dec = codec.Decoder(files[kind][0], dev, use_graph=use_graph)
                torch.cuda.synchronize()
                label = f"{kind}, {'graph' if use_graph else 'eager'}" + (" (first of the process)" if r == 0 else "")
                ready.setdefault(label, []).append(time.time() - t0)
                del dec
    for label, v in ready.items():
        print(f"c1 pruned model-ready, {label}: {min(v) * 1e3:.1f} ms best, {max(v) * 1e3:.1f} worst of {len(v)}")
    plans = {}
    for kind, fmt, cls in (("dense", qstream, ops.HuffDequant), ("sparse", zstream, ops.HuffzDequant)):
        fs = fmt.read(files[kind][0])
        items = []
        for r in fs.records:
            tdt = torch.float16 if r.dtype == qstream.F16 else torch.float32
            items.append((torch.empty(r.count, device=dev), torch.from_numpy(r.min).to(dev).to(tdt), torch.from_numpy(r.scale).to(dev).to(tdt), r.red, r.inner, r.run_bits))
        plans[kind] = cls(fs.words, fs.lengths, items)
        plans[kind].launch().check()
    times = time_graph([plans["dense"].launch, plans["sparse"].launch], reps=20, rounds=max(rounds, 5))
    for (kind, plan), (best, worst) in zip(plans.items(), times):
        plan.check()
        n = files[kind][1]["n_symbols"]
        print(f"c1 pruned decode kernel, {kind}: {best:.1f} us best, {worst:.1f} worst per launch ({plan.n_runs} runs, {n / best:.0f} elements/us, "
              f"{files[kind][1]['symbol_bits'] / 8 / best / 1e3:.2f} GB/s of coded bytes in)")
    (db, dw), (sb, sw) = times
    print(f"c1 pruned decode kernel: sparse - dense = {sb - db:+.1f} us best against best; the dense kernel's own worst - best spread is {dw - db:.1f} us")


def run_chunked(case, n_frames, rounds):
    import torch
    from boosting_nerv_amd import bitstream, codec, ops, rstream
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    from boosting_nerv_amd.synth import SyntheticVideo
    dev = torch.device("cuda:0")
    args, model = build(case)
    model = model.to(dev)
    model.init_data()
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    frames = None
    if args.model == "HNeRV_Boost":
        vid = SyntheticVideo(n_frames, h, w)
        frames = torch.stack([vid.frame(i, device=dev) for i in range(n_frames)])
        with torch.no_grad():
            model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    args.full_data_length = n_frames
    buf = io.BytesIO()
    v1 = codec.encode(model, DiffEntropyModel("gaussian"), args, frames, buf)
    del model
    files = {"version 1": buf.getvalue()}
    print(f"{case}: {args.model} {h}x{w}, {n_frames} frames; version-1 file {codec.describe(v1)}", flush=True)
    for run in (256, 1024):
        out = io.BytesIO()
        t0 = time.time()
        b = codec.repack(files["version 1"], out, run)
        files[f"chunked {run}"] = out.getvalue()
        extra = b["ans_words"] + b["run_index"] + b["padding"] - v1["coded_words"] - 32 * (b["n_tensors"] + b["n_embeds"])      # (a version-1 record carries its word count)
        print(f"{case} chunked, run {run}: repack {time.time() - t0:.2f} s on the host; file {codec.describe_chunked(b)}; {b['bytes'] - v1['bytes']:+d} bytes "
              f"against version 1 ({100.0 * (b['bytes'] - v1['bytes']) / v1['bytes']:+.2f} %), {extra / b['n_symbols']:.4f} bits per symbol for cutting "
              f"({(b['ans_words'] - v1['coded_words']) / b['n_symbols']:.4f} in the words, {b['run_index'] / b['n_symbols']:.4f} in the run index)", flush=True)

    # (1) model-ready, the kinds alternated
    first = {}
    for label, blob in files.items():                          # (code objects, lazily built tables: the first construction of each kind apart)
        torch.cuda.synchronize()
        t0 = time.time()
        dec = codec.Decoder(blob, dev, use_graph=False)
        torch.cuda.synchronize()
        first[label] = time.time() - t0
        print(f"{case} model-ready, first construction, {label}: {first[label] * 1e3:.1f} ms", flush=True)
    ready = {}
    for r in range(max(rounds, 3)):
        for use_graph in (False, True):
            for label, blob in files.items():
                t0 = time.time()
                (bitstream if label == "version 1" else rstream).read(blob)
                t_read = time.time() - t0
                dec = None                                     # (the previous decoder is released outside the timed window)
                torch.cuda.synchronize()
                t0 = time.time()
                dec = codec.Decoder(blob, dev, use_graph=use_graph)
                torch.cuda.synchronize()
                key = (label, "graph" if use_graph else "eager")
                ready.setdefault(key, []).append((time.time() - t0, t_read))
                print(f"{case} round {r} model-ready, {key[1]}, {label}: {ready[key][-1][0] * 1e3:.1f} ms (container parse + CRC alone: {t_read * 1e3:.1f} ms)", flush=True)
    ref = codec.Decoder(files["version 1"], dev, use_graph=False)
    for label, blob in files.items():
        d = codec.Decoder(blob, dev, use_graph=False)
        assert all(torch.equal(d.decode_f32(i), ref.decode_f32(i)) for i in (0, n_frames - 1)), label
    for mode in ("eager", "graph"):
        base = min(t for t, _ in ready[("version 1", mode)])
        for label in files:
            v = [t for t, _ in ready[(label, mode)]]
            print(f"{case} model-ready, {mode}, {label}: {min(v) * 1e3:.1f} ms best, {max(v) * 1e3:.1f} worst of {len(v)} (version 1 / this = {base / min(v):.2f})")

    # the decode launch alone: the same tables, outputs of its own
    for run in (256, 1024):
        rs = rstream.read(files[f"chunked {run}"])
        items = [(torch.empty(r.count, device=dev), float(r.scale), r.lo, r.hi, float(r.mean), float(r.std), r.run_words, None if r.beta is None else float(r.beta))
                 for r in rs.tensors + rs.embeds]
        t0 = time.time()
        plan = ops.AnsDequant(rs.words, items, run)
        t_plan = time.time() - t0
        plan.launch().check()
        (best, worst), = time_graph([plan.launch], reps=50, rounds=max(rounds, 3))
        plan.check()
        n_sym = sum(r.count for r in rs.tensors + rs.embeds)
        print(f"{case} decode launch, run {run}: {best:.1f} us best, {worst:.1f} worst per launch ({plan.n_runs} runs in {plan.n_blocks} blocks, "
              f"{n_sym / best:.0f} symbols/us, {4 * rs.words.size / best / 1e3:.2f} GB/s of words in, {4 * n_sym / best / 1e3:.1f} GB/s of fp32 out); "
              f"tables, descriptors and uploads on the host: {t_plan * 1e3:.1f} ms")


WIDE_SPAN = 25000


def build_wide(wide):
    """The seeded c1q model on the device with init_data() scales; wide: the scale of its first (stem) weight quantiser cut so that the
    record spans about WIDE_SPAN values.  -> (args, model, entropy model)."""
    import torch
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    args, model = build("c1q")
    model = model.to("cuda:0")
    model.init_data()
    if wide:
        with torch.no_grad():
            model._quant_modules()[0].weight_quantizer.scale.mul_(255.0 / WIDE_SPAN)
    return args, model, DiffEntropyModel("gaussian")


def run_wide(n_frames, rounds):
    import torch
    from boosting_nerv_amd import bitstream, codec, estream, ops, wstream
    dev = torch.device("cuda:0")
    for wide in (False, True):
        args, model, em = build_wide(wide)
        args.full_data_length = n_frames
        buf = io.BytesIO()
        codec.encode(model, em, args, None, buf)
        v1 = buf.getvalue()
        label = f"c1q, stem weight on about {WIDE_SPAN} values" if wide else "c1q"
        for run in (256, 1024):
            out = io.BytesIO()
            b = codec.repack(v1, out, run, tables="empirical", wide=True)
            ws = wstream.read(out.getvalue())
            recs = ws.tensors + ws.embeds
            print(f"{label}, run {run}: BNRV {len(v1)} bytes, BNRW {b['bytes']} bytes ({100.0 * (b['bytes'] - len(v1)) / len(v1):+.2f} %); "
                  f"{b['n_wide_records']} wide records, largest shift {b['max_shift']}, {b['n_table_records']} of {len(recs)} under a table", flush=True)
            plans = []
            if wide:
                r0, m0 = recs[0], bitstream.read(v1).tensors[0]
                spans = wstream.record_words(ws)
                side = 8 * (18 + (8 if r0.model == estream.GAUSSIAN else len(estream.table_bytes(r0.freq))) + 2 * r0.run_words.size)
                print(f"{label}, run {run}: the wide record: {r0.count} symbols on {r0.hi - r0.lo + 1} values, shift {r0.shift}, model {r0.model}: "
                      f"{32 * spans[0][1]} bits of words + {side} bits of side, table and run index = {(32 * spans[0][1] + side) / r0.count:.3f} bits per symbol | "
                      f"its version-1 message: {32 * m0.words.size} bits of words + {8 * 28} of side = {(32 * m0.words.size + 224) / r0.count:.3f} bits per symbol",
                      flush=True)
            else:
                es_blob = io.BytesIO()
                codec.repack(v1, es_blob, run, tables="empirical")
                es = estream.read(es_blob.getvalue())
                assert all(r.shift == 0 for r in recs) and (es.words == ws.words).all()
                plans.append(("ops.AnsDequantTables", ops.AnsDequantTables(es.words, [(torch.empty(r.count, device=dev), float(r.scale), r.lo, estream.record_cdf(r), r.run_words,
                                                                                     None if r.beta is None else float(r.beta)) for r in es.tensors + es.embeds], run)))
            plans.append(("ops.AnsDequantWide", ops.AnsDequantWide(ws.words, [(torch.empty(r.count, device=dev), float(r.scale), r.lo, r.hi, wstream.record_cdf(r), r.shift,
                                                                               r.run_words, None if r.beta is None else float(r.beta)) for r in recs], run)))
            for _, p in plans:
                p.launch().check()
            times = time_graph([p.launch for _, p in plans], reps=50, rounds=max(rounds, 3))
            n_sym = sum(r.count for r in recs)
            for (name, p), (best, worst) in zip(plans, times):
                p.check()
                print(f"{label} decode launch, run {run}, {name}: {best:.1f} us best, {worst:.1f} worst per launch = {best / run:.3f} us per symbol of a run "
                      f"({p.n_runs} runs in {p.n_blocks} blocks, {n_sym / best:.0f} symbols/us)", flush=True)
        if wide:                                               # the file decodes to the model of its version-1 file
            a, b = codec.Decoder(out.getvalue(), dev, use_graph=False), codec.Decoder(v1, dev, use_graph=False)
            assert a.kind == "wide" and all(torch.equal(x, y) for x, y in zip(a.model.state_dict().values(), b.model.state_dict().values()))
            assert torch.equal(a.decode_f32(0), b.decode_f32(0))
            print(f"{label}: the BNRW file decodes to the parameters and the first frame of its version-1 file", flush=True)
        del model


def run_temporal(n_frames, rounds):
    import numpy as np
    import torch
    from kencode import consecutive_frames
    from boosting_nerv_amd import codec, ops, tstream, wstream
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    dev = torch.device("cuda:0")
    args, model = build("c5")
    model = model.to(dev)
    model.init_data()
    h, w = (int(v) for v in args.crop_list.split("_")[:2])
    frames = consecutive_frames(n_frames, h, w, dev)
    with torch.no_grad():
        model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    args.full_data_length = n_frames
    em = DiffEntropyModel("gaussian")
    buf = io.BytesIO()
    codec.encode(model, em, args, frames, buf)
    v1 = buf.getvalue()
    label = f"c5 seeded, frames 100..{100 + n_frames - 1}"
    for run in (256, 1024):
        fw, ft = io.BytesIO(), io.BytesIO()
        bw = codec.encode(model, em, args, frames, fw, run=run, tables="empirical", wide=True)
        bt = codec.encode(model, em, args, frames, ft, run=run, tables="empirical", wide=True, temporal=True)
        fw, ft = fw.getvalue(), ft.getvalue()
        print(f"{label}, run {run}: BNRV {len(v1)} bytes, BNRW {bw['bytes']} bytes, BNRT {bt['bytes']} bytes, {bt['n_inter_frames']} of {bt['n_embeds']} frames as differences",
              flush=True)
        ready = {"wide": [], "temporal": []}
        for _ in range(max(rounds, 3) + 1):                    # (the first pair apart: code objects)
            for kind, blob in (("wide", fw), ("temporal", ft)):
                torch.cuda.synchronize()
                t0 = time.time()
                dec = codec.Decoder(blob, dev, use_graph=False)
                torch.cuda.synchronize()
                ready[kind].append(time.time() - t0)
                assert dec.kind == kind
                del dec
        print(f"{label}, run {run}: Decoder ready (file bytes in memory -> model and embeddings on the device, eager frame loop): wide {min(ready['wide'][1:]) * 1e3:.1f} ms "
              f"best, {max(ready['wide'][1:]) * 1e3:.1f} worst of {len(ready['wide']) - 1} | temporal {min(ready['temporal'][1:]) * 1e3:.1f} ms best, "
              f"{max(ready['temporal'][1:]) * 1e3:.1f} worst (first calls {ready['wide'][0] * 1e3:.0f}, {ready['temporal'][0] * 1e3:.0f} ms)", flush=True)
        ts, ws = tstream.read(ft), wstream.read(fw)
        n_t, P = len(ts.tensors), int(np.prod(ts.embed_shape))
        at = sum(n for _, n in wstream.record_words(ts)[:n_t])
        item = lambda r, out: (out, float(r.scale), r.lo, r.hi, wstream.record_cdf(r), r.shift, r.run_words, None if r.beta is None else float(r.beta))      # noqa: E731
        held, out = torch.empty(n_frames, P, dtype=torch.int32, device=dev), torch.empty(n_frames, P, device=dev)
        plans = [("ops.AnsDequantWide, the whole wide file", ops.AnsDequantWide(ws.words, [item(r, torch.empty(r.count, device=dev)) for r in ws.tensors + ws.embeds], run)),
                 ("ops.AnsDequantWide, tensor records", ops.AnsDequantWide(ts.words[:at], [item(r, torch.empty(r.count, device=dev)) for r in ts.tensors], run)),
                 ("ops.AnsDecodeWide, embedding records", ops.AnsDecodeWide(ts.words[at:], [(held[i], r.lo, r.hi, wstream.record_cdf(r), r.shift, r.run_words)
                                                                                             for i, r in enumerate(ts.embeds)], run)),
                 ("ops.EmbedChainDequant", ops.EmbedChainDequant(held, ts.preds, [float(r.scale) for r in ts.embeds], [float(r.beta) for r in ts.embeds], out))]
        for _, p in plans:
            p.launch().check()
        q = torch.from_numpy(tstream.decode_embeds(ts)).to(dev)
        assert torch.equal(out, q.float() * float(ts.embeds[0].scale) + float(ts.embeds[0].beta))      # (one scale and beta for the clip)
        times = time_graph([p.launch for _, p in plans], reps=50, rounds=max(rounds, 3))
        for (name, p), (best, worst) in zip(plans, times):
            p.check()
            print(f"{label} decode launch, run {run}, {name}: {best:.1f} us best, {worst:.1f} worst per launch", flush=True)
    a, b = codec.Decoder(ft, dev, use_graph=False), codec.Decoder(v1, dev, use_graph=False)
    assert a.kind == "temporal" and all(torch.equal(x, y) for x, y in zip(a.model.state_dict().values(), b.model.state_dict().values()))
    assert torch.equal(a.embeds, b.embeds) and torch.equal(a.decode_f32(0), b.decode_f32(0)) and torch.equal(a.decode_f32(n_frames - 1), b.decode_f32(n_frames - 1))
    print(f"{label}: the BNRT file decodes to the parameters, the embeddings and the first and last frame of its version-1 file", flush=True)


def run_posthoc_temporal(n_frames, rounds):
    import numpy as np
    import torch
    from kencode import describe_posthoc_pair, h1_posthoc
    from boosting_nerv_amd import codec, ops, pstream, qstream
    dev = torch.device("cuda:0")
    model, args, records, quant_embed = h1_posthoc(n_frames, dev)
    fq, fp = io.BytesIO(), io.BytesIO()
    bq = codec.encode_posthoc(model, args, records, quant_embed, fq)
    bp = codec.encode_posthoc(model, args, records, quant_embed, fp, temporal=True)
    fq, fp = fq.getvalue(), fp.getvalue()
    label = f"H1 seeded, frames 100..{100 + n_frames - 1} at 1080p"
    describe_posthoc_pair(label, bq, bp)
    ready = {"posthoc": [], "posthoc_temporal": []}
    for _ in range(max(rounds, 3) + 1):                        # (the first pair apart: code objects)
        for kind, blob in (("posthoc", fq), ("posthoc_temporal", fp)):
            torch.cuda.synchronize()
            t0 = time.time()
            dec = codec.Decoder(blob, dev, use_graph=False)
            torch.cuda.synchronize()
            ready[kind].append(time.time() - t0)
            assert dec.kind == kind
            del dec
    a, b = ready["posthoc"], ready["posthoc_temporal"]
    print(f"{label}: Decoder ready (file bytes in memory -> model and embeddings on the device, eager frame loop): .bnrq {min(a[1:]) * 1e3:.1f} ms best, "
          f"{max(a[1:]) * 1e3:.1f} worst of {len(a) - 1} | .bnrp {min(b[1:]) * 1e3:.1f} ms best, {max(b[1:]) * 1e3:.1f} worst (first calls {a[0] * 1e3:.0f}, "
          f"{b[0] * 1e3:.0f} ms)", flush=True)
    qs, ps = qstream.read(fq), pstream.read(fp)
    e = ps.embeds
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    item = lambda r: (torch.empty(r.count, device=dev), up(r.min), up(r.scale), r.red, r.inner, r.run_bits)      # noqa: E731
    P = int(np.prod(e.shape[1:]))
    held, out = torch.empty(n_frames, P, dtype=torch.uint8, device=dev), torch.empty(n_frames, P, device=dev)
    plans = [("ops.HuffDequant, the whole .bnrq file", ops.HuffDequant(qs.words, qs.lengths, [item(r) for r in qs.records])),
             ("ops.HuffDequant, tensor section", ops.HuffDequant(ps.words, ps.lengths, [item(r) for r in ps.records]))]
    for kind, lengths, words, name in ((pstream.INTRA, e.lengths0, e.words0, "intra"), (pstream.INTER, e.lengths1, e.words1, "inter")):
        rows = np.flatnonzero(e.pred == kind)
        if rows.size:
            plans.append((f"ops.HuffDecodeU8, {rows.size} {name} frames", ops.HuffDecodeU8(words, lengths, [(held[int(t)], e.run_bits[int(t)]) for t in rows])))
    plans.append(("ops.EmbedChainDequantU8", ops.EmbedChainDequantU8(held, e.pred, up(e.min), up(e.scale), e.red, e.inner, out)))
    plans.append(("ops.EmbedDeltaU8 (encoder)", ops.EmbedDeltaU8(quant_embed["quant"].reshape(n_frames, -1))))
    for _, p in plans:
        p.launch().check()
    assert np.array_equal(pstream.decode_embeds(ps), quant_embed["quant"].reshape(n_frames, -1).cpu().numpy())
    times = time_graph([p.launch for _, p in plans], reps=50, rounds=max(rounds, 3))
    for (name, p), (best, worst) in zip(plans, times):
        p.check()
        print(f"{label} launch, {name}: {best:.1f} us best, {worst:.1f} worst per launch", flush=True)
    a, b = codec.Decoder(fp, dev, use_graph=False), codec.Decoder(fq, dev, use_graph=False)
    assert a.kind == "posthoc_temporal" and all(torch.equal(x, y) for x, y in zip(a.model.state_dict().values(), b.model.state_dict().values()))
    assert torch.equal(a.embeds, b.embeds) and torch.equal(a.embeds.view(n_frames, -1), out)
    assert torch.equal(a.decode_f32(0), b.decode_f32(0)) and torch.equal(a.decode_f32(n_frames - 1), b.decode_f32(n_frames - 1))
    print(f"{label}: the .bnrp file decodes to the parameters, the embeddings and the first and last frame of its .bnrq file", flush=True)


def forward_rates(cfg):
    """Decode (forward-only) rate of a bench.py decoder (c1 | c3 | c4) on the HIP path: frames/s for single-frame decodes under
    torch.no_grad(), eager and as a captured hipGraph (N4 row: the figure the reference logs as "FPS" in evaluate())."""
    import torch
    import bench
    dev = torch.device("cuda:0")
    args, model = bench.build(cfg)
    model = model.to(dev).eval()
    N = 132
    idx = torch.tensor([[37 / N]], dtype=torch.float64, device=dev).reshape(1)
    with torch.no_grad():
        for _ in range(5):
            out = model(idx, norm_idx=idx)[0]
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(100):
            out = model(idx, norm_idx=idx)[0]
        torch.cuda.synchronize()
        print(f"eager decode : {100 / (time.time() - t0):8.1f} frames/s")
        g = torch.cuda.CUDAGraph(); s = torch.cuda.Stream()
        from boosting_nerv_amd import _lib as L
        with torch.cuda.stream(s):
            L.ctx()                                  # the capture stream's library context (and its scratch) must exist before the capture
            with torch.cuda.graph(g, stream=s):
                out = model(idx, norm_idx=idx)[0]
        g.replay(); torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(300):
            g.replay()
        torch.cuda.synchronize()
        print(f"graph decode : {300 / (time.time() - t0):8.1f} frames/s   ({(time.time() - t0) / 300 * 1e3:.3f} ms/frame)")
        # engine.DecodeGraph: the same captured forward with the decoder's weight fragments prepared once (context plan, ABI 4)
        from boosting_nerv_amd.engine import DecodeGraph
        embed = model(idx, norm_idx=idx)[1][0]
        dg = DecodeGraph(model, idx, embed, idx)
        ref = model(idx, embed, norm_idx=idx)[0]
        assert torch.equal(dg(idx, embed, idx)[0], ref)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(300):
            dg.graph.replay()
        torch.cuda.synchronize()
        print(f"DecodeGraph  : {300 / (time.time() - t0):8.1f} frames/s   ({(time.time() - t0) / 300 * 1e3:.3f} ms/frame), {dg.wplan_entries} planned weight tensors")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cfg", nargs="?", default="c1", help="without --bitstream: the bench.py recipe whose forward-only rate is measured")
    ap.add_argument("--bitstream", action="store_true", help="time the bitstream decoder instead")
    ap.add_argument("--posthoc", action="store_true", help="with --bitstream: the post-hoc quantised file of the regression path (C1 model)")
    ap.add_argument("--chunked", action="store_true", help="with --bitstream: the version-1 CEM file against the chunked file of the same model (c1q, c5)")
    ap.add_argument("--wide", action="store_true", help="with --bitstream: the decode kernel of the wide kind against the narrow one (c1q)")
    ap.add_argument("--temporal", action="store_true", help="with --bitstream: the temporal kind against the wide kind of the same run (c5); with --posthoc: the temporal post-hoc kind against .bnrq (H1)")
    ap.add_argument("--sparse", action="store_true", help="with --bitstream --posthoc: the sparse file against the dense file of the same pruned C1 model")
    ap.add_argument("--sparsity", type=float, default=0.4, help="with --sparse: the global magnitude sparsity the model is pruned to")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["c1q", "c5", "pack"], default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kdecode needs the GPU"
    if not a.bitstream:
        forward_rates(a.cfg)
        return 0
    if a.posthoc and a.temporal:
        run_posthoc_temporal(a.frames, a.rounds)
        return 0
    if a.posthoc and a.sparse:
        run_posthoc_sparse(a.frames, a.rounds, a.sparsity)
        return 0
    if a.posthoc:
        run_posthoc(a.frames, a.rounds)
        return 0
    if a.wide:
        run_wide(a.frames, a.rounds)
        return 0
    if a.temporal:
        run_temporal(a.frames, a.rounds)
        return 0
    if a.chunked:
        for case in ([a.only] if a.only else ["c1q", "c5"]):
            run_chunked(case, a.frames, a.rounds)
        return 0
    for case in ([a.only] if a.only else ["c1q", "c5", "pack"]):
        if case == "pack":
            run_pack(a.rounds)
        else:
            run_case(case, a.frames, a.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
