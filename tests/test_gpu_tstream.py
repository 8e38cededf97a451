"""The temporal CEM file on the GPU (``-m gpu``): the difference kernel against int64 numpy, the integer-output decode
against the host decoder, the chain kernel against its two-operation numpy restatement, the file codec.encode(..., temporal=True) writes
against the host repack of the version-1 file of the same model, its decode against the version-1 decode frame for frame, and the command
line.  Every operand starts one element past a 16-byte boundary."""
import io
import os

import numpy as np
import pytest
import torch

from oracle import configs
from tstream_cases import chain_reference, check_bound, delta_reference
from wstream_cases import record, tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows(a, pitch, dtype=torch.int32, fill=0):
    """A [N, P] view with row pitch `pitch` that starts one element past a 16-byte boundary, holding `a` (None: `fill`)."""
    N, P = a if isinstance(a, tuple) else a.shape
    buf = torch.full((N * pitch + 2,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0 and pitch >= P
    view = buf[1:1 + N * pitch].view(N, pitch)[:, :P]
    if not isinstance(a, tuple):
        view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and (N == 1 or view.stride(0) == pitch)
    return buf, view


# ---------------------------------------------------------------------------------------------------------------------- differences
@pytest.mark.parametrize("N", [1, 2, 5])
def test_embed_delta_is_exact_against_int64_numpy(N):
    """Every P in one test per N: 1, 63, 64, 65 (around a wave of quads and the tail of up to three elements), 576 (the tiny model's), 2307
    (more than one block of quads, tail 3); values up to +-2^27, so the differences reach 2^28 and the sum of squares wraps 2^64; padded
    row pitches of either parity, so the rows of q and of d meet every 4-byte phase of a 16-byte line."""
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(N)
    for P in (1, 63, 64, 65, 576, 2307):
        q = rng.integers(-(1 << 27), (1 << 27) + 1, size=(N, P)).astype(np.int32)
        q[0, 0], q[-1, -1] = 1 << 27, -(1 << 27)
        _, qd = _rows(q, P + 3)
        dbuf, dd = _rows((N, P), P + 6, fill=-77)
        job = ops.EmbedDelta(qd, dd).launch().check()
        lo, hi, s1, s2 = job.host()
        d, wlo, whi, ws1, ws2 = delta_reference(q)
        assert torch.equal(dd[1:].cpu(), torch.from_numpy(d[1:].astype(np.int32))), (N, P)
        assert (dd[0] == -77).all().item() and dbuf[0].item() == -77 and dbuf[-1].item() == -77       # row 0 and the guards are not written
        if N > 1:
            assert (dbuf[1:1 + N * (P + 6)].view(N, P + 6)[:, P:] == -77).all().item()                  # nor the padding of a row
        assert s2.dtype == np.uint64 and np.array_equal(lo, wlo) and np.array_equal(hi, whi) and np.array_equal(s1, ws1) and np.array_equal(s2, ws2), (N, P)
        if N > 1 and P == 2307:
            assert int(np.abs(d).max()) > 1 << 27                          # (the sums above did wrap: the case is not idle)
            job.launch()                                                   # relaunchable: the statistics are zeroed by every launch
            assert all(np.array_equal(a, b) for a, b in zip(job.host(), (lo, hi, s1, s2)))
    # d allocated by the op; a dense q
    q = rng.integers(-9, 10, size=(max(N, 2), 130)).astype(np.int32)
    job = ops.EmbedDelta(torch.from_numpy(q).to(DEV)).launch()
    assert torch.equal(job.d[1:].cpu(), torch.from_numpy(q[1:] - q[:-1]))
    with pytest.raises(ValueError, match="dense rows"):
        ops.EmbedDelta(torch.zeros(4, 8, dtype=torch.int32, device=DEV).t())
    with pytest.raises(ValueError, match="dense rows"):
        ops.EmbedDelta(torch.zeros(4, 8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- integer decode
@pytest.mark.parametrize("run", [64, 256])
def test_ans_decode_wide_equals_the_host_decoder(run):
    """Records of wstream_cases at shift 0 and shifts 1, 3 and 9 under both models, sizes around a run and a block of 64 runs, one launch."""
    from boosting_nerv_amd import ops, wstream
    from boosting_nerv_amd.lib import entropy_model as em
    plan = [(3000, 2 * run + 5, 0), (3000, 1, 1), (4097, 63, 0), (4097, run + 1, 1), (25457, 64 * run + 5, 1), ((1 << 20) + 1, 4097, 0), (61, 577, 1)]
    recs, words = [], []
    for j, (span, n, model) in enumerate(plan):
        sym, lo, hi, k = record(span, n, 10 * run + j)
        cdf = tables(sym, lo, hi, k)[model]
        w, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, run)
        recs.append(wstream.WRecord(n, np.float32(1.0), lo, hi, model, k, *((None, None, np.diff(cdf.astype(np.int64)).astype(np.uint32)) if model else
                                                                             (np.float32(sym.mean()), np.float32(max(sym.std(), 1.0)), None)), rw))
        words.append(w)
    assert sorted({r.shift for r in recs}) == [0, 1, 3, 9]
    ws = wstream.WStream(dict(ans_run=run), recs, [], None, [], np.concatenate(words))
    outs = [torch.full((r.count + 2,), -5, dtype=torch.int32, device=DEV) for r in recs]
    assert all(o[1:-1].data_ptr() % 16 == 4 for o in outs)
    ops.AnsDecodeWide(ws.words, [(o[1:-1], r.lo, r.hi, wstream.record_cdf(r), r.shift, r.run_words) for o, r in zip(outs, recs)], run).launch().check()
    for k, (o, r) in enumerate(zip(outs, recs)):
        want = wstream.decode_record(ws, k)
        assert want.dtype == np.int32 and torch.equal(o[1:-1].cpu(), torch.from_numpy(want)), (k, r.count, r.shift)
        assert o[0].item() == -5 and o[-1].item() == -5
    with pytest.raises(ValueError, match="int32"):
        ops.AnsDecodeWide(ws.words, [(o[1:-1].float(), r.lo, r.hi, wstream.record_cdf(r), r.shift, r.run_words) for o, r in zip(outs, recs)], run)
    # a payload that does not match its run index is flagged, as by the float kernel
    bad = ws.words.copy()
    bad[int(recs[0].run_words[0]) - 1] ^= 0x00010000           # the high state word of the first run (a damaged bulk word may go unnoticed: rANS resynchronises)
    with pytest.raises(ValueError, match="did not consume"):
        ops.AnsDecodeWide(bad, [(o[1:-1], r.lo, r.hi, wstream.record_cdf(r), r.shift, r.run_words) for o, r in zip(outs, recs)], run).launch().check()


# ---------------------------------------------------------------------------------------------------------------------- chain
def _patterns(N):
    pats = {"intra": [0] * N, "inter": [0] + [1] * (N - 1), "alternating": [t % 2 for t in range(N)]}
    if N > 2:
        pats["cut at 1"] = [0, 0] + [1] * (N - 2)
        pats["cut at N-1"] = [0] + [1] * (N - 2) + [0]
    return pats


@pytest.mark.parametrize("N", [1, 2, 7, 8, 9, 63, 64, 65, 130])
def test_embed_chain_dequant_equals_its_numpy_restatement(N):
    """N at the kernel's unroll (BNERV_CHAIN_UNROLL = 8) and at the frames a block serves (BNERV_CHAIN_SEG = 64), each minus 1, at it and plus 1;
    130: a third segment that starts in the middle of a chain.  P = 257 and 577: more than one block along p, neither a multiple of 64."""
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import ops
    assert (L.CHAIN_UNROLL, L.CHAIN_SEG) == (8, 64)
    rng = np.random.default_rng(N)
    for P in (257, 577) if N in (9, 65) else (257,):
        sym = rng.integers(-300, 301, size=(N, P)).astype(np.int32)
        scale = rng.uniform(1e-3, 0.1, size=N).astype(np.float32)
        beta = rng.normal(size=N).astype(np.float32)
        _, sd = _rows(sym, P + 5)
        for name, pred in _patterns(N).items():
            obuf, od = _rows((N, P), P + 2, dtype=torch.float32, fill=float("nan"))
            ops.EmbedChainDequant(sd, pred, scale, beta, od).launch().check()
            q, want = chain_reference(sym, pred, scale, beta)
            assert want.dtype == np.float32 and torch.equal(od.cpu(), torch.from_numpy(want)), (N, P, name)
            assert torch.isnan(obuf[0]).item() and torch.isnan(obuf[-1]).item()
            if N > 1:
                assert torch.isnan(obuf[1:1 + N * (P + 2)].view(N, P + 2)[:, P:]).all().item()      # the padding of a row is not written


def test_a_chain_that_leaves_int32_is_flagged_and_arguments_are_validated_before_a_launch():
    from boosting_nerv_amd import ops
    N, P = 70, 130
    sym = np.zeros((N, P), dtype=np.int32)
    sym[0] = (1 << 31) - 70                                   # 69 steps of +1 end on 2^31 - 1: the last int32
    sym[1:] = 1
    pred = [0] + [1] * (N - 1)
    ones = np.ones(N, np.float32)
    _, sd = _rows(sym, P + 1)
    _, od = _rows((N, P), P + 1, dtype=torch.float32)
    ops.EmbedChainDequant(sd, pred, ones, 0 * ones, od).launch().check()
    assert od[-1, 0].item() == float(np.float32((1 << 31) - 1))
    sym[40, 17] = 2                                           # one element passes 2^31, in the second block's frames
    _, sd = _rows(sym, P + 1)
    job = ops.EmbedChainDequant(sd, pred, ones, 0 * ones, od).launch()
    with pytest.raises(ValueError, match="leaves int32"):
        job.check()
    sym[0] = -sym[0] - 2
    sym[1:] = -1
    _, sd = _rows(sym, P + 1)
    with pytest.raises(ValueError, match="leaves int32"):
        ops.EmbedChainDequant(sd, pred, ones, 0 * ones, od).launch().check()
    with pytest.raises(ValueError, match="frame 0 is predicted"):
        ops.EmbedChainDequant(sd, [1] * N, ones, ones, od)
    with pytest.raises(ValueError, match="0 \\| 1"):
        ops.EmbedChainDequant(sd, [0, 2] + [0] * (N - 2), ones, ones, od)
    with pytest.raises(ValueError, match="entries each"):
        ops.EmbedChainDequant(sd, pred, ones[:-1], ones[:-1], od)
    with pytest.raises(ValueError, match="out is"):
        ops.EmbedChainDequant(sd, pred, ones, ones, od[:-1])


# ---------------------------------------------------------------------------------------------------------------------- file against file
N_FRAMES, HW = 8, (180, 320)
_shared = {}


def _clip():
    """[f10, f11, 1 - f12, uniform noise, f13, flip(f13), f14, zeros] of SyntheticVideo(64, 180, 320): consecutive frames, a negative, noise,
    a mirror image and a black frame."""
    from boosting_nerv_amd.synth import SyntheticVideo
    vid = SyntheticVideo(64, *HW)
    f = {i: vid.frame(i) for i in (10, 11, 12, 13, 14)}
    noise = torch.rand(3, *HW, generator=torch.Generator().manual_seed(5))
    return torch.stack([f[10], f[11], 1 - f[12], noise, f[13], torch.flip(f[13], dims=[-1]), f[14], torch.zeros(3, *HW)])


def _encoded():
    """One tiny quantised HNeRV_Boost, built as tests/test_gpu_wstream.py builds it (first weight record cut to span about 25 000 values), its
    version-1 file, and the temporal and wide files at run 64 and 256 under both tables, coded on the device."""
    if _shared:
        return _shared
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    from boosting_nerv_amd.train_nerv_all import build_model
    args = configs.tiny_hnerv_quant()
    torch.manual_seed(3)
    model = build_model(args).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
    model.init_data()
    with torch.no_grad():
        next(iter(model._quant_modules())).weight_quantizer.scale.mul_(255.0 / 25000.0)
    frames = _clip().to(DEV)
    em = DiffEntropyModel("gaussian")
    with torch.no_grad():
        model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    v1 = io.BytesIO()
    codec.encode(model, em, args, frames, v1)
    files = {}
    for run in (64, 256):
        for tables_ in ("gaussian", "empirical"):
            t, w = io.BytesIO(), io.BytesIO()
            bt = codec.encode(model, em, args, frames, t, run=run, tables=tables_, wide=True, temporal=True)
            bw = codec.encode(model, em, args, frames, w, run=run, tables=tables_, wide=True)
            files[run, tables_] = (t.getvalue(), bt, w.getvalue(), bw)
    assert model.training                                  # (the mode is put back)
    _shared.update(v1=v1.getvalue(), files=files, model=model, em=em, args=args, frames=frames)
    return _shared


@pytest.mark.parametrize("tables_", ["gaussian", "empirical"])
@pytest.mark.parametrize("run", [64, 256])
def test_device_encode_temporal_writes_the_bytes_of_the_host_repack(run, tables_):
    """With a seeded untrained encoder the host coder at run 256 gave the modes I P I P I P P I on this clip; only the two wide margins are
    asserted: frame 1 after its neighbour is inter (2464 against 4640 bits), the black frame is intra (256 against 4640 bits)."""
    from boosting_nerv_amd import codec, estream, tstream, wstream
    ref = _encoded()
    blob, budget, wide_blob, wide_budget = ref["files"][run, tables_]
    host = io.BytesIO()
    host_budget = codec.repack(ref["v1"], host, run, tables_, wide=True, temporal=True)
    ts = tstream.read(blob)
    per_frame = [32 * int(r.run_words.sum()) for r in ts.embeds]
    print(f"run {run}, {tables_}: modes {''.join('IP'[p] for p in ts.preds)}, words per frame {per_frame}, BNRT {len(blob)} bytes, BNRW {len(wide_blob)} bytes; "
          f"BNRW words per frame {[32 * int(r.run_words.sum()) for r in wstream.read(wide_blob).embeds]}")
    assert blob[:4] == b"BNRT" and blob == host.getvalue() and budget == host_budget == tstream.info(blob) == codec.info(blob)
    assert budget["total"] == 8 * len(blob) == sum(budget[k] for k in estream.ITEMS) and budget["ans_run"] == run and budget["n_embeds"] == N_FRAMES
    assert ts.preds[0] == 0 and ts.preds[1] == 1 and ts.preds[7] == 0, ts.preds
    assert budget["n_inter_frames"] == sum(ts.preds) and budget["n_wide_records"] == 1 and budget["max_shift"] == 3
    check_bound(budget, wide_budget)
    assert wide_budget == wstream.info(wide_blob)
    # what the file holds resolves to the symbols of the version-1 file
    from boosting_nerv_amd import bitstream
    from boosting_nerv_amd.lib.entropy_model import ans_decode_gaussian
    v1 = bitstream.read(ref["v1"])
    want = np.stack([ans_decode_gaussian(r.words, r.count, r.lo, r.hi, float(r.mean), float(r.std)) for r in v1.embeds])
    assert np.array_equal(tstream.decode_embeds(ts), want)
    if (run, tables_) == (256, "gaussian"):
        with pytest.raises(ValueError, match="wide=True"):
            codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], io.BytesIO(), run=run, temporal=True)


def test_encode_temporal_refuses_a_model_without_frame_embeddings():
    from boosting_nerv_amd import codec
    with pytest.raises(ValueError, match="HNeRV_Boost"):
        codec.encode(None, None, configs.tiny_nerv(), None, io.BytesIO(), run=256, wide=True, temporal=True)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_temporal_file_decodes_to_the_frames_of_the_version_1_file(use_graph):
    from boosting_nerv_amd import codec
    ref = _encoded()
    b = codec.Decoder(io.BytesIO(ref["v1"]), DEV, use_graph=use_graph)
    for key in ((256, "empirical"), (64, "gaussian")) if not use_graph else ((256, "empirical"),):
        a = codec.Decoder(io.BytesIO(ref["files"][key][0]), DEV, use_graph=use_graph)
        assert (a.kind, b.kind) == ("temporal", "cem") and len(a) == len(b) == N_FRAMES and a.frame_hw == b.frame_hw == HW
        assert a.settings["embed_pred"] == "prev"
        for (ka, va), (kb, vb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        assert torch.equal(a.embeds, b.embeds)
        for i in (2, 0, 7, 1, 3, 6, 5, 4):
            assert torch.equal(a.decode_f32(i), b.decode_f32(i)), (key, i)
        for x, y in zip(a, b):                             # the pipelined uint8 iterator
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------- command line
def _pack_ref(x):
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_cli_train_with_bitstream_temporal_then_info_and_decode(tmp_path, monkeypatch, capsys):
    """train_nerv_compression --bitstream tiny.bnrt --bitstream_run 256 --bitstream_temporal on the README's 4-frame recipe: the file is the new
    kind, the logged line is its budget, `codec info` adds up to 8 * size, `codec decode` writes the frames of the version-1 file of the same run."""
    from PIL import Image
    from boosting_nerv_amd import codec, estream, tstream
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    path, v1_path = str(tmp_path / "tiny.bnrt"), str(tmp_path / "tiny.bnrv")
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
             "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 "
             "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
             "-e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
             "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1 "
             f"--bitstream {path} --bitstream_run 256 --bitstream_temporal")
    seen = {}
    orig_eval = C.evaluate

    def spy(model, loader, rank, args, *a, **k):
        out = orig_eval(model, loader, rank, args, *a, **k)
        seen["args"] = args
        if k.get("write_bitstream"):                       # the version-1 file of the same run, from the same evaluation's model
            codec.encode(model, k["entropy_model"], args, loader, v1_path)
        return out
    monkeypatch.setattr(C, "evaluate", spy)
    C.main(flags.split())
    size = os.path.getsize(path)
    assert open(path, "rb").read(4) == tstream.MAGIC
    budget = tstream.info(path)
    assert seen["args"].bitstream_budget == budget and budget["total"] == 8 * size and budget["ans_run"] == 256 and budget["n_embeds"] == 4
    assert budget["ans_tables"] == "gaussian" and budget["n_table_records"] == 0 and budget["n_inter_frames"] + budget["n_intra_frames"] == 4
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    line = [x for x in log.splitlines() if x.startswith("Bitstream ")]
    assert len(line) == 1 and line[0].rstrip() == f"Bitstream {path}: {codec.describe_temporal(budget)}"
    capsys.readouterr()
    assert codec.main(["info", path]) == budget
    printed = capsys.readouterr().out
    assert f"{size} bytes = {8 * size} bits" in printed and "temporal: " in printed and sum(budget[k] for k in estream.ITEMS) == 8 * size
    host = io.BytesIO()
    codec.repack(v1_path, host, 256, wide=True, temporal=True)
    assert host.getvalue() == open(path, "rb").read()
    out_dir = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(out_dir)]) == 4
    names = sorted(os.listdir(out_dir))
    assert names == [f"frame_{i:04d}.png" for i in range(4)]
    dec, dec1 = codec.Decoder(path, DEV), codec.Decoder(v1_path, DEV)
    assert (dec.kind, dec1.kind) == ("temporal", "cem")
    for i, n in enumerate(names):
        img = Image.open(out_dir / n)
        assert img.size == (320, 180) and img.mode == "RGB"
        assert torch.equal(dec.decode_f32(i), dec1.decode_f32(i))
        assert np.array_equal(np.asarray(img), _pack_ref(dec1.decode_f32(i))[0].cpu().numpy())
