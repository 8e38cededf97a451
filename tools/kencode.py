"""File sizes and encode times of the chunked CEM file with per-record tables (estream.py) on the HIP path.

    python tools/kencode.py [--only c1q|c5] [--frames 16] [--rounds 3]     seeded weights (the cases of tools/kdecode.py)
    python tools/kencode.py --trained tiny|c1 [--epochs E]                 a trained model: sizes only
    python tools/kencode.py --wide [--rounds 3]                            the wide kind (BNRW) on c1q: kernels against the narrow ones
    python tools/kencode.py --temporal [--frames 16] [--rounds 3]          the temporal kind (BNRT) against the wide kind on c5: sizes, encode times
    python tools/kencode.py --temporal --trained tiny|c5 [--frames 16] [--epochs E]     the same sizes of a trained model
    python tools/kencode.py --posthoc [--epochs E]                         the temporal post-hoc kind (BNRP) against .bnrq / .bnrz: sizes

Seeded cases, in ONE process:
  sizes   the version-1 file (BNRV), the chunked file (BNRC) and the file with per-record tables (BNRE) at runs 256 and 1024; how many
          records took a table; the BNRE file of the device path against the host repack of the version-1 file, byte for byte;
  time    codec.encode(run=N) -- the host chain: version-1 messages, decoded again, re-encoded in runs -- against
          codec.encode(run=N, tables="empirical") -- histogram, encode and compaction launches on the device -- alternated, host clock,
          every call ending in a device synchronisation; then the three launches alone (ops.SymHist, ops.AnsEncodeRuns, ops.AnsCompact
          with everything uploaded), each captured `reps` times into a graph of its own and the graphs replayed in turn under HIP events.
--trained tiny: the README's tiny compression recipe (HNeRV_Boost, 4 frames of 180x320) through train_nerv_compression.main with --bitstream.
--trained c1:   the C1 model (NeRV_Boost 1.5M, 132 synthetic 720x1280 frames): train_nerv_all.main for --epochs epochs (regression), then
                train_nerv_compression.main from that checkpoint (--weight) for --epochs // 2 rate-distortion epochs with the compression
                recipe's quantiser and rate flags (without --embed_entropy: the model has no embedding to code) and --bitstream.
--wide: the encode kernel of the wide kind (wstream.py) on the seeded c1q model in ONE process: the narrow model's records
under ops.AnsEncodeRuns and, with shift 0, under ops.AnsEncodeRunsWide (both tables per record, as the file is coded); then the model of
tools/kdecode.py --wide, whose stem weight record spans about 25 000 values, under ops.AnsEncodeRunsWide with ops.SymHistWide; the file of
codec.encode(..., wide=True) against the host repack, byte for byte.
--temporal: the temporal kind (tstream.py) against the wide kind of the same run and tables on the seeded c5 model and --frames
CONSECUTIVE frames (100, 101, ...) of the 600-frame 1080p synthetic clip: codec.encode(..., wide=True) and (..., temporal=True) alternated, host
clock, every call ending in a device synchronisation; the temporal file against the host repack byte for byte; the bound of the choice rule;
embedding bits per frame (words, record bytes, pred byte) and how many frames are coded as differences.  With --trained tiny: the README's
tiny recipe; with --trained c5: the C3 regression recipe for --epochs epochs on --frames frames, then one rate-distortion epoch of the c5 recipe
from that checkpoint -- sizes from the version-1 file either way.
--posthoc: the temporal POST-HOC file (pstream.py) against the .bnrq and .bnrz file of the same evaluation, sizes only: the
README's tiny HNeRV recipe trained for --epochs epochs (train_nerv_all.main --bitstream, then --eval_only for the other kinds), and the seeded
H1 model (regression/bunny/hnerv.sh's HNeRV with the strides 5 3 2 2 2 of the 1080p recipes: a 16 x 9 x 16 embedding) over 16 and 64 CONSECUTIVE
frames of the 600-frame 1080p synthetic clip; per file the bytes, the frames coded as differences and the bits of an intra and an inter frame.
Both --trained cases write the version-1 file; the other kinds are made from it on the host (codec.repack: the bytes of the device path, tests/test_gpu_estream.py).
(needs the GPU)"""
import argparse
import glob
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RUNS = (256, 1024)
TINY = ("--outf kenc --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
        "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 "
        "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
        "-e 2 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
        "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2")

# the compression flags of the recipes on a model that decodes from the frame index (no embedding to code: no --embed_entropy)
C1_CEM = ("--quant --quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta "
          "--lr 0.0005 --lr_type cosine_0_1_0.1 --lambda_rate 0.05 --target_bit 4")


def sizes_from_v1(label, v1):
    """BNRC and BNRE of a version-1 file at every run, on the host; one line each."""
    from boosting_nerv_amd import bitstream, codec
    b1 = bitstream.info(v1)
    print(f"{label}: BNRV {len(v1)} bytes ({b1['n_tensors']} tensors, {b1['n_embeds']} embeddings, coded words {b1['coded_words']} bits)", flush=True)
    bs = bitstream.read(v1)
    wide = [(r.count, r.lo, r.hi, float(r.scale)) for r in bs.tensors + bs.embeds if r.hi - r.lo + 1 > 4096]
    if wide:                                                   # (the chunked kinds carry at most 4096 symbol values per record: section 27)
        print(f"{label}: no chunked file of either kind: {len(wide)} of {len(bs.tensors + bs.embeds)} records span more than 4096 symbol values "
              f"(symbols, lo, hi, scale): {wide[:6]}", flush=True)
        return b1
    for run in RUNS:
        c, e = io.BytesIO(), io.BytesIO()
        bc = codec.repack(v1, c, run)
        be = codec.repack(v1, e, run, tables="empirical")
        report(label, run, len(v1), bc, be)
    return b1


def report(label, run, n_v1, bc, be):
    n_rec = be["n_tensors"] + be["n_embeds"]
    part = lambda b: b["ans_words"] + b.get("tables", 0) + b["tensor_side"] + b["embed_side"]      # noqa: E731
    assert part(be) <= part(bc) + 8 * n_rec
    print(f"{label} run {run}: BNRC {bc['bytes']} bytes ({100.0 * (bc['bytes'] - n_v1) / n_v1:+.2f} % against BNRV) | BNRE {be['bytes']} bytes "
          f"({100.0 * (be['bytes'] - n_v1) / n_v1:+.2f} % against BNRV, {100.0 * (be['bytes'] - bc['bytes']) / bc['bytes']:+.2f} % against BNRC); "
          f"{be['n_table_records']} of {n_rec} records took a table ({be['tables']} bits of tables); words + tables + side: BNRE {part(be)} bits, BNRC {part(bc)} bits",
          flush=True)


def run_seeded(case, n_frames, rounds, reps):
    import numpy as np
    import torch
    from kdecode import build, time_graph
    from boosting_nerv_amd import codec, estream, ops
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel, ans_counts_cdf, ans_gaussian_cdf
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
    em = DiffEntropyModel("gaussian")
    buf = io.BytesIO()
    codec.encode(model, em, args, frames, buf)
    v1 = buf.getvalue()
    print(f"{case}: {args.model} {h}x{w}, {n_frames} frames, seeded weights", flush=True)
    sizes_from_v1(case, v1)

    def encode(run, tables):
        out = io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.time()
        codec.encode(model, em, args, frames, out, run=run, tables=tables)
        torch.cuda.synchronize()
        return time.time() - t0, out.getvalue()

    for run in RUNS:                                            # first calls apart (code objects, lazily built tables); the bytes compared
        t_h, chunked = encode(run, "gaussian")
        t_d, emp = encode(run, "empirical")
        host = io.BytesIO()
        codec.repack(v1, host, run, tables="empirical")
        assert emp == host.getvalue(), (case, run)
        print(f"{case} run {run}: first calls: host chain {t_h * 1e3:.0f} ms, device path {t_d * 1e3:.0f} ms; the device path's file is the host repack's, "
              f"byte for byte", flush=True)
    times = {}
    for r in range(rounds):
        for run in RUNS:
            for tables in ("gaussian", "empirical"):
                times.setdefault((run, tables), []).append(encode(run, tables)[0])
    for run in RUNS:
        g, e = times[(run, "gaussian")], times[(run, "empirical")]
        print(f"{case} encode, run {run}: host chain codec.encode(run=N) {min(g) * 1e3:.0f} ms best, {max(g) * 1e3:.0f} worst of {len(g)} | device path "
              f"tables='empirical' {min(e) * 1e3:.0f} ms best, {max(e) * 1e3:.0f} worst | host chain / device path = {min(g) / min(e):.2f}", flush=True)

    # the three launches alone: the symbols of the file, both tables per record, everything uploaded
    for run in RUNS:
        es = estream.read(encode(run, "empirical")[1])
        recs = es.tensors + es.embeds
        syms = [torch.from_numpy(estream.decode_record(es, k)).to(dev) for k in range(len(recs))]
        hist = ops.SymHist([(s, r.lo, r.hi - r.lo + 1) for s, r in zip(syms, recs)]).launch().check()
        counts = hist.host()
        items = []
        for s, r, c in zip(syms, recs, counts):
            assert np.array_equal(c, np.bincount(s.cpu().numpy() - r.lo, minlength=r.hi - r.lo + 1))
            # two items per record, as the encoder launches: its Gaussian and its own table.  A record that took its table carries no
            # (mean, std): the Gaussian of its symbols' moments stands in for the one of its codes' (same alphabet, nearly the same words)
            sf = s.float()
            g = estream.record_cdf(r) if r.model == estream.GAUSSIAN else ans_gaussian_cdf(r.lo, r.hi, float(sf.mean()), max(float(sf.std()), 1e-5))
            items += [(s, r.lo, g), (s, r.lo, ans_counts_cdf(c))]
        enc = ops.AnsEncodeRuns(items, run).launch().check()
        rw = enc.run_words()
        comp = enc.compact(list(range(0, len(items), 2)), rw).launch().check()
        (h_lo, h_hi), (k_lo, k_hi), (e_lo, e_hi), (c_lo, c_hi) = time_graph([hist.launch, lambda: hist.launch(zero=False), enc.launch, comp.launch], reps=reps,
                                                                            rounds=max(rounds, 3))
        n_sym = sum(r.count for r in recs)
        print(f"{case} launches, run {run}: histogram {h_lo:.1f} us with the memset of its counts (worst {h_hi:.1f}), {k_lo:.1f} us the kernel alone (worst {k_hi:.1f}; "
              f"{hist.n_blocks} blocks, {n_sym / k_lo:.0f} symbols/us) | encode under both "
              f"tables {e_lo:.1f} us (worst {e_hi:.1f}; {enc.n_slots} runs in {enc.n_blocks} blocks, {2 * n_sym / e_lo:.0f} symbols/us) | compaction {c_lo:.1f} us "
              f"(worst {c_hi:.1f}; {comp.n_out} words)", flush=True)
        hist.check(), enc.check(), comp.check()


def run_wide(n_frames, rounds, reps):
    import numpy as np
    import torch
    from kdecode import build_wide, time_graph
    from boosting_nerv_amd import codec, ops, wstream
    from boosting_nerv_amd.lib.entropy_model import ans_counts_cdf
    dev = torch.device("cuda:0")
    for wide in (False, True):
        args, model, em = build_wide(wide)
        args.full_data_length = n_frames
        buf = io.BytesIO()
        codec.encode(model, em, args, None, buf)
        v1 = buf.getvalue()
        label = "c1q, stem weight on about 25000 values" if wide else "c1q"
        for run in RUNS:
            out, host = io.BytesIO(), io.BytesIO()
            torch.cuda.synchronize()
            t0 = time.time()
            b = codec.encode(model, em, args, None, out, run=run, tables="empirical", wide=True)
            torch.cuda.synchronize()
            t_d = time.time() - t0
            assert codec.repack(v1, host, run, tables="empirical", wide=True) == b and host.getvalue() == out.getvalue()
            print(f"{label}, run {run}: codec.encode(wide=True) {t_d * 1e3:.0f} ms (a first call); BNRV {len(v1)} bytes, BNRW {b['bytes']} bytes "
                  f"({100.0 * (b['bytes'] - len(v1)) / len(v1):+.2f} %), {b['n_wide_records']} wide records, largest shift {b['max_shift']}; the device path's file "
                  f"is the host repack's, byte for byte", flush=True)
            ws = wstream.read(out.getvalue())
            recs = ws.tensors + ws.embeds
            syms = [torch.from_numpy(wstream.decode_record(ws, k)).to(dev) for k in range(len(recs))]
            hist = ops.SymHistWide([(s, r.lo, r.hi, r.shift) for s, r in zip(syms, recs)]).launch().check()
            counts = hist.host()
            items, narrow = [], []
            for s, r, c in zip(syms, recs, counts):
                assert np.array_equal(c, np.bincount((s.cpu().numpy() - r.lo) >> r.shift, minlength=c.size))
                sf = s.float()                                 # (a record that took its table carries no moments: those of its symbols stand in)
                g = wstream.record_cdf(r) if r.mean is not None else wstream.record_cdf(r._replace(model=0, mean=float(sf.mean()), std=max(float(sf.std()), 1e-5)))
                items += [(s, r.lo, r.hi, g, r.shift), (s, r.lo, r.hi, ans_counts_cdf(c), r.shift)]
                narrow += [(s, r.lo, g), (s, r.lo, items[-1][3])]
            plans = [("ops.AnsEncodeRunsWide", ops.AnsEncodeRunsWide(items, run).launch().check())]
            if not wide:
                plans.insert(0, ("ops.AnsEncodeRuns", ops.AnsEncodeRuns(narrow, run).launch().check()))
                a, b2 = plans[0][1].result(), plans[1][1].result()
                assert np.array_equal(a[0], b2[0])             # shift 0: the narrow encoder's words
            times = time_graph([lambda: hist.launch(zero=False)] + [p.launch for _, p in plans], reps=reps, rounds=max(rounds, 3))
            n_sym = sum(r.count for r in recs)
            print(f"{label} launches, run {run}: ops.SymHistWide {times[0][0]:.1f} us the kernel alone (worst {times[0][1]:.1f}; {n_sym / times[0][0]:.0f} symbols/us)", flush=True)
            for (name, p), (best, worst) in zip(plans, times[1:]):
                p.check()
                print(f"{label} encode launch under both tables, run {run}, {name}: {best:.1f} us best, {worst:.1f} worst = {best / run:.3f} us per symbol of a run "
                      f"({p.n_slots} runs in {p.n_blocks} blocks, slots of {p.slot_words} words, {2 * n_sym / best:.0f} symbols/us)", flush=True)
        del model


def embed_bits(stream):
    """Bits per frame of the embedding records of a wide or temporal stream: their words, their serialised records, the pred byte."""
    from boosting_nerv_amd import codec
    pred = 8 if hasattr(stream, "preds") else 0
    return sum(32 * int(r.run_words.sum()) + 8 * codec._record_bytes(r) + pred for r in stream.embeds) / max(len(stream.embeds), 1)


def temporal_sizes(label, v1, runs=RUNS):
    """BNRT against BNRW of a version-1 file at every run under both tables, on the host (the bytes of the device path); one line each."""
    from boosting_nerv_amd import codec, tstream, wstream
    part = lambda b: b["ans_words"] + b["tables"] + b["tensor_side"] + b["embed_side"]      # noqa: E731
    for run in runs:
        for tables in ("gaussian", "empirical"):
            w, t = io.BytesIO(), io.BytesIO()
            bw = codec.repack(v1, w, run, tables, wide=True)
            bt = codec.repack(v1, t, run, tables, wide=True, temporal=True)
            assert part(bt) <= part(bw) + 8 * bt["n_embeds"], (part(bt), part(bw))
            ew, et = embed_bits(wstream.read(w.getvalue())), embed_bits(tstream.read(t.getvalue()))
            print(f"{label} run {run}, {tables}: BNRW {bw['bytes']} bytes | BNRT {bt['bytes']} bytes ({100.0 * (bt['bytes'] - bw['bytes']) / bw['bytes']:+.2f} %); "
                  f"{bt['n_inter_frames']} of {bt['n_embeds']} frames as differences; embedding bits per frame: BNRW {ew:.0f}, BNRT {et:.0f} "
                  f"({100.0 * (et - ew) / ew:+.1f} %); words + tables + side: BNRT {part(bt)} bits, BNRW {part(bw)} bits", flush=True)


def consecutive_frames(n_frames, h, w, dev, first=100, clip=600):
    import torch
    from boosting_nerv_amd.synth import SyntheticVideo
    vid = SyntheticVideo(clip, h, w)
    return torch.stack([vid.frame(first + i, device=dev) for i in range(n_frames)])


def run_temporal(n_frames, rounds):
    import torch
    from kdecode import build
    from boosting_nerv_amd import codec
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
    label = f"c5 seeded, frames 100..{100 + n_frames - 1} of synthetic:uvg"
    print(f"{label}: {args.model} {h}x{w}, BNRV {len(v1)} bytes", flush=True)
    temporal_sizes(label, v1)

    def encode(run, tables, temporal):
        out = io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.time()
        codec.encode(model, em, args, frames, out, run=run, tables=tables, wide=True, temporal=temporal)
        torch.cuda.synchronize()
        return time.time() - t0, out.getvalue()

    for run in RUNS:
        for tables in ("gaussian", "empirical"):
            host = io.BytesIO()
            codec.repack(v1, host, run, tables, wide=True, temporal=True)
            assert encode(run, tables, True)[1] == host.getvalue(), (run, tables)
        print(f"{label} run {run}: the device path's BNRT file is the host repack's, byte for byte, under both tables", flush=True)
    times = {}
    for _ in range(rounds):
        for run in RUNS:
            for temporal in (False, True):
                times.setdefault((run, temporal), []).append(encode(run, "empirical", temporal)[0])
    for run in RUNS:
        a, b = times[(run, False)], times[(run, True)]
        print(f"{label} encode, run {run}, tables='empirical' (the {n_frames} encoder forwards included): wide {min(a) * 1e3:.0f} ms best, {max(a) * 1e3:.0f} worst of "
              f"{len(a)} | temporal {min(b) * 1e3:.0f} ms best, {max(b) * 1e3:.0f} worst", flush=True)


def run_trained_temporal(which, epochs, n_frames):
    import torch
    import bench
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd import train_nerv_compression as C
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            path = os.path.join(tmp, "trained.bnrv")
            if which == "tiny":
                C.main(TINY.split() + ["--bitstream", path])
                label = "tiny recipe, trained (2 epochs)"
            else:
                data = ["--data_path", f"synthetic:{n_frames}x1080x1920", "--vid", "c5", "--not_resume"]
                T.main(bench.RECIPES["c3"]["flags"].split() + data + ["--outf", "kenc_reg", "-e", str(epochs), "--eval_freq", str(epochs)])
                ckpt = glob.glob(os.path.join(tmp, "output", "kenc_reg", "**", "model_latest.pth"), recursive=True)
                assert len(ckpt) == 1, ckpt
                C.main(bench.RECIPES["c5"]["flags"].split() + data + ["--outf", "kenc_cem", "-e", "1", "--eval_freq", "1", "--weight", ckpt[0], "--bitstream", path])
                label = f"c5, {epochs} regression epochs (C3 recipe) + 1 rate-distortion epoch on {n_frames} frames"
            torch.cuda.synchronize()
            temporal_sizes(label, open(path, "rb").read())
        finally:
            os.chdir(cwd)


def run_trained(which, epochs, cem_epochs=None):
    import torch
    import bench
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd import train_nerv_compression as C
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            path = os.path.join(tmp, "trained.bnrv")
            if which == "tiny":
                C.main(TINY.split() + ["--bitstream", path])
                label = "tiny recipe, trained (2 epochs)"
            else:
                r = bench.RECIPES["c1"]
                flags = r["flags"].split() + ["--data_path", f"synthetic:{r['n']}x{r['h']}x{r['w']}", "--vid", "c1", "--not_resume"]
                T.main(flags + ["--outf", "kenc_reg", "-e", str(epochs), "--eval_freq", str(epochs)])
                ckpt = glob.glob(os.path.join(tmp, "output", "kenc_reg", "**", "model_latest.pth"), recursive=True)
                assert len(ckpt) == 1, ckpt
                cem = max(epochs // 2, 1) if cem_epochs is None else cem_epochs
                C.main(flags + C1_CEM.split() + ["--outf", "kenc_cem", "-e", str(cem), "--eval_freq", str(cem), "--weight", ckpt[0], "--bitstream", path])
                label = f"C1, {epochs} regression + {cem} compression epochs on {r['n']} frames"
            torch.cuda.synchronize()
            sizes_from_v1(label, open(path, "rb").read())
        finally:
            os.chdir(cwd)


def h1_posthoc(n_frames, dev, sparse=False):
    """The seeded H1 model at 1080p with evaluate()'s records for its post-hoc twin over n_frames consecutive frames -> (model, args, records,
    quant_embed)."""
    import copy
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hnerv_ref
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import quant_tensor
    args = copy.copy(hnerv_ref.h1_args())
    args.__dict__.update(enc_strds=[5, 3, 2, 2, 2], dec_strds=[5, 3, 2, 2, 2], quant_model_bit=8, quant_embed_bit=6, crop_list="1080_1920",
                         final_size=1080 * 1920, full_data_length=n_frames, batchSize=1, bitstream_sparse=sparse)
    torch.manual_seed(1)
    model = T.build_model(args).to(dev)
    frames = consecutive_frames(n_frames, 1080, 1920, dev)
    with torch.no_grad():
        (plain, _), records = T.quant_model(model, args)
        plain.eval()
        embeds = [plain(frames[i:i + 1], None, norm_idx=torch.tensor([(i + 1) / n_frames], dtype=torch.float64, device=dev))[1][0] for i in range(n_frames)]
        quant_embed, _ = quant_tensor(torch.cat(embeds, 0), args.quant_embed_bit)
    return model, args, records, quant_embed


def describe_posthoc_pair(label, plain, temporal):
    """One line: a temporal budget (pstream.info) against the budget of the plain file of the same records."""
    per = lambda bits, n: f"{bits / n:.0f}" if n else "-"      # noqa: E731
    extra = temporal["embed_symbol_bits"] + temporal["embed_run_index"] + temporal["embed_side"] + temporal["embed_tables"]
    print(f"{label}: plain {plain['bytes']} bytes, temporal {temporal['bytes']} bytes (ratio {temporal['bytes'] / plain['bytes']:.4f}); "
          f"{temporal['n_inter_frames']} of {temporal['n_inter_frames'] + temporal['n_intra_frames']} frames as differences; code bits per frame: intra "
          f"{per(temporal['intra_frame_bits'], temporal['n_intra_frames'])}, inter {per(temporal['inter_frame_bits'], temporal['n_inter_frames'])}; "
          f"embedding section {extra} bits of {temporal['total']}", flush=True)


def run_posthoc(epochs):
    import torch
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    dev = torch.device("cuda:0")
    recipe = ("--model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
              "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 --lr 0.001 --data_path synthetic:4x180x320 --vid tiny --crop_list 180_320 --resize_list -1 --modelsize 0.05 "
              f"--lower_width 6 -b 1 --eval_freq {epochs} -p 2 -e {epochs} --outf t")
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            T.main((recipe + " --not_resume --bitstream t.bnrp --bitstream_temporal").split())
            T.main((recipe + " --eval_only --bitstream t.bnrq").split())
            T.main((recipe + " --eval_only --bitstream s.bnrp --bitstream_sparse --bitstream_temporal").split())
            T.main((recipe + " --eval_only --bitstream s.bnrz --bitstream_sparse").split())
            budgets = {k: codec.info(os.path.join(tmp, k)) for k in ("t.bnrp", "t.bnrq", "s.bnrp", "s.bnrz")}
        finally:
            os.chdir(here)
    describe_posthoc_pair(f"tiny HNeRV recipe, {epochs} epochs, dense (.bnrq)", budgets["t.bnrq"], budgets["t.bnrp"])
    describe_posthoc_pair(f"tiny HNeRV recipe, {epochs} epochs, sparse (.bnrz)", budgets["s.bnrz"], budgets["s.bnrp"])
    for n in (16, 64):
        for sparse in (False, True):
            model, args, records, quant_embed = h1_posthoc(n, dev, sparse)
            plain, temporal = io.BytesIO(), io.BytesIO()
            bp = codec.encode_posthoc(model, args, records, quant_embed, plain)
            bt = codec.encode_posthoc(model, args, records, quant_embed, temporal, temporal=True)
            describe_posthoc_pair(f"H1 seeded, frames 100..{100 + n - 1} at 1080p, {'sparse (.bnrz)' if sparse else 'dense (.bnrq)'}", bp, bt)
            print(f"    {codec.describe_any(bt)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c1q", "c5"], default=None)
    ap.add_argument("--trained", choices=["tiny", "c1", "c5"], default=None, help="c5: with --temporal only")
    ap.add_argument("--temporal", action="store_true", help="the temporal kind against the wide kind (c5; with --trained: tiny or c5)")
    ap.add_argument("--posthoc", action="store_true", help="the temporal post-hoc kind (BNRP) against .bnrq / .bnrz: tiny recipe trained, H1 seeded")
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--cem_epochs", type=int, default=None, help="--trained c1: rate-distortion epochs (default: --epochs // 2)")
    ap.add_argument("--wide", action="store_true", help="the encode kernels of the wide kind against the narrow ones (c1q)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kencode needs the GPU"
    if a.posthoc:
        run_posthoc(a.epochs)
        return 0
    if a.temporal:
        if a.trained:
            assert a.trained in ("tiny", "c5"), "--temporal --trained takes tiny or c5 (C1 has no frame embeddings)"
            run_trained_temporal(a.trained, a.epochs, a.frames)
        else:
            run_temporal(a.frames, a.rounds)
        return 0
    assert a.trained != "c5", "--trained c5 needs --temporal"
    if a.wide:
        run_wide(a.frames, a.rounds, a.reps)
        return 0
    if a.trained:
        run_trained(a.trained, a.epochs, a.cem_epochs)
        return 0
    for case in ([a.only] if a.only else ["c1q", "c5"]):
        run_seeded(case, a.frames, a.rounds, a.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
