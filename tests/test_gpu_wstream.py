"""The wide chunked CEM file on the GPU (``-m gpu``): the bucket histogram against np.bincount, the device encoder
against the host coder of the same library bit for bit, the decode kernel against float(sym) * scale (+ beta), the file
codec.encode(..., wide=True) writes against the host repack of the version-1 file of the same model, its decode against the version-1 decode
frame for frame, and the command line.  Every operand starts one element past a 16-byte boundary."""
import io
import os

import numpy as np
import pytest
import torch

from oracle import configs
from wstream_cases import SIZES, SPANS, check_word_bound, min_shift, record, tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(sym):
    """int32 symbols on the device, starting one element past a 16-byte boundary."""
    buf = torch.zeros(sym.size + 1, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = torch.from_numpy(sym)
    out = buf[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---------------------------------------------------------------------------------------------------------------------- histogram
def test_sym_hist_wide_equals_bincount_of_the_buckets():
    """Every size on every span, a narrow record (shift 0) and one of three slices, in ONE launch."""
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import ops
    host = [record(span, n, 7 * n + span) for span in SPANS for n in SIZES]
    host.insert(3, record(3000, 12, 1))
    host.insert(4, record(25457, 2 * L.HIST_SLICE + 777, 2))
    assert sorted({k for _, _, _, k in host}) == [0, 1, 2, 3, 9]
    got = ops.sym_hist_wide([(_dev(s), lo, hi, k) for s, lo, hi, k in host])
    assert len(got) == len(host)
    for j, ((s, lo, hi, k), g) in enumerate(zip(host, got)):
        B = (hi - lo + (1 << k)) >> k
        assert g.dtype == np.uint32 and g.size == B <= 4096 and np.array_equal(g, np.bincount((s - lo) >> k, minlength=B)), (j, s.size, k)
    # the object is relaunchable: the counts are zeroed by every launch
    s, lo, hi, k = host[4]
    job = ops.SymHistWide([(_dev(s), lo, hi, k)])
    job.launch().launch().check()
    assert np.array_equal(job.host()[0], np.bincount((s - lo) >> k, minlength=3183))


def test_a_symbol_outside_its_range_is_flagged_and_arguments_are_validated_before_a_launch():
    """An error flag, never an address: the histogram does not count it, the encoder's lane stops writing."""
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.lib import entropy_model as em
    sym, lo, hi, k = record(4097, 300, 5)
    bad = sym.copy()
    bad[130], bad[131] = hi + 1, lo - 1                     # hi + 1 would still fall into the last bucket
    job = ops.SymHistWide([(_dev(bad), lo, hi, k), (_dev(sym), lo, hi, k)]).launch()
    with pytest.raises(ValueError, match="outside"):
        job.check()
    counts = job.host()
    assert np.array_equal(counts[0], np.bincount((np.delete(bad, (130, 131)) - lo) >> k, minlength=2049)) and int(counts[1].sum()) == 300
    cdf = tables(sym, lo, hi, k)[0]
    enc = ops.AnsEncodeRunsWide([(_dev(bad), lo, hi, cdf, k), (_dev(sym), lo, hi, cdf, k)], 64).launch()
    with pytest.raises(ValueError, match="outside its range"):
        enc.check()
    rw, want = enc.run_words(), em.ans_encode_wide_runs(sym, lo, hi, cdf, k, 64)[1]
    assert rw[0][2] == 0 and np.array_equal(np.delete(rw[0], 2), np.delete(want, 2)) and np.array_equal(rw[1], want)
    d = _dev(sym)
    for items, what in (([(d, lo, hi, cdf, 17)], "shift"), ([(d, lo, hi, cdf, k + 1)], "buckets"), ([(d, lo, hi, cdf[:-1], k)], "buckets"),
                        ([(d, lo, lo + 8191, cdf, 0)], "buckets"), ([(d.float(), lo, hi, cdf, k)], "int32")):
        with pytest.raises(ValueError, match=what):
            ops.AnsEncodeRunsWide(items, 64)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.AnsEncodeRunsWide([(d, lo, hi, cdf, k)], 100)
    with pytest.raises(ValueError, match="buckets"):
        ops.SymHistWide([(d, lo, hi, 0)])
    out = torch.empty(300, device=DEV)
    words, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, 64)
    with pytest.raises(ValueError, match="run lengths"):
        ops.AnsDequantWide(words, [(out, 1.0, lo, hi, cdf, k, rw[:-1], None)], 64)
    with pytest.raises(ValueError, match="add up"):
        ops.AnsDequantWide(words[:-1], [(out, 1.0, lo, hi, cdf, k, rw, None)], 64)
    with pytest.raises(ValueError, match="rise strictly"):
        ops.AnsDequantWide(words, [(out, 1.0, lo, hi, np.concatenate([cdf[:5], cdf[4:-1]]), k, rw, None)], 64)


# ---------------------------------------------------------------------------------------------------------------------- encoder, decoder
_coded = {}


def _cases(run):
    """One launch at `run` -> [(symbols, lo, hi, shift, cdf, scale, beta, host words, host run_words)]: shifts 0, 1, 2, 3 and 9 under both
    models; a record of 64 * run + 5 symbols (a second block of one record, its last run of 5); a record of 64 runs of uniform symbols at
    shift 9, 20 bits each -- at run 256 and above its block's words outgrow the 8192 the kernel stages; the sizes 1, 63, 64, 65, 4097."""
    if run in _coded:
        return _coded[run]
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(run)
    plan = [(25457, 64 * run + 5, 1), ((1 << 20) + 1, 64 * run, 0), (3000, 2 * run + 5, 0), (3000, 1, 1), (4097, 63, 0), (4097, run + 1, 1),
            (25457, 65, 0), ((1 << 20) + 1, 4097, 1), (8193, 64, 1), (8193, 4097, 0)]
    out = []
    for j, (span, n, model) in enumerate(plan):
        sym, lo, hi, k = record(span, n, 100 * run + j)
        if j == 1:
            sym = rng.integers(lo, hi + 1, size=n).astype(np.int32)
            sym[0], sym[-1] = lo, hi
        cdf = tables(sym, lo, hi, k)[model]
        words, rw = em.ans_encode_wide_runs(sym, lo, hi, cdf, k, run)
        check_word_bound(rw, n, run, k)
        out.append((sym, lo, hi, k, cdf, float(np.float32(rng.uniform(1e-5, 0.1))), None if j % 3 else float(np.float32(rng.normal())), words, rw))
    assert sorted({c[3] for c in out}) == [0, 1, 2, 3, 9]
    assert (int(out[1][8].sum()) > 8192) == (run >= 256)      # the block that outgrows the staged span
    _coded[run] = out
    return out


@pytest.mark.parametrize("run", [64, 256, 4096])
def test_ans_encode_runs_wide_equals_the_host_coder_bit_for_bit(run):
    from boosting_nerv_amd import ops
    cases = _cases(run)
    enc = ops.AnsEncodeRunsWide([(_dev(c[0]), c[1], c[2], c[4], c[3]) for c in cases], run).launch().check()
    assert enc.slot_words == run * (24 + 9) // 32 + 3
    words, run_words = enc.result()
    assert words.dtype == np.uint32 and len(run_words) == len(cases)
    for j, (c, got) in enumerate(zip(cases, run_words)):
        assert got.dtype == np.uint16 and np.array_equal(got, c[8]), (j, c[0].size, c[3])
    assert np.array_equal(words, np.concatenate([c[7] for c in cases]))
    # a chosen subset, in another order: the runs of those items alone
    words, run_words = enc.result([6, 0, 3])
    assert np.array_equal(words, np.concatenate([cases[j][7] for j in (6, 0, 3)])) and all(np.array_equal(a, cases[j][8]) for a, j in zip(run_words, (6, 0, 3)))


@pytest.mark.parametrize("run", [64, 256, 4096])
def test_ans_dequant_wide_gives_float_sym_times_scale_plus_beta(run):
    from boosting_nerv_amd import ops
    cases = _cases(run)
    outs = [torch.full((c[0].size + 2,), float("nan"), device=DEV) for c in cases]
    assert all(o[1:-1].data_ptr() % 16 == 4 for o in outs)
    ops.ans_dequant_wide(np.concatenate([c[7] for c in cases]), [(o[1:-1], c[5], c[1], c[2], c[4], c[3], c[8], c[6]) for o, c in zip(outs, cases)], run)
    for j, (o, c) in enumerate(zip(outs, cases)):
        want = torch.from_numpy(c[0]).to(DEV).float() * c[5]
        if c[6] is not None:
            want = want + c[6]
        assert torch.equal(o[1:-1], want), (j, c[0].size, c[3])
        assert torch.isnan(o[0]).item() and torch.isnan(o[-1]).item()


# ---------------------------------------------------------------------------------------------------------------------- file against file
def _quant(a):
    a.__dict__.update(quant=True, quant_model_bit=8, quant_bias_bit=8, quant_embed_bit=8, per_channel_w=False, per_channel_b=False,
                      per_channel_e=False, quantizer_w="scale", quantizer_b="scale", quantizer_e="scalebeta", embed_entropy=True)
    return a


_CONFIGS = {"HNeRV_Boost": configs.tiny_hnerv_quant, "NeRV_Boost": lambda: _quant(configs.tiny_nerv())}
N_FRAMES, HW, RUN = 4, (180, 320), 256
_shared = {}


def _encoded(name):
    """One tiny quantised model per architecture, built as tests/test_gpu_estream.py builds it; then the scale of its first weight
    quantiser is cut so that the record spans about 25 000 values.  Its version-1 file and the wide files, coded on the device."""
    if name in _shared:
        return _shared[name]
    from boosting_nerv_amd import codec
    from boosting_nerv_amd.lib.entropy_model import DiffEntropyModel
    from boosting_nerv_amd.train_nerv_all import build_model
    args = _CONFIGS[name]()
    torch.manual_seed(3)
    model = build_model(args).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
    model.init_data()
    with torch.no_grad():
        next(iter(model._quant_modules())).weight_quantizer.scale.mul_(255.0 / 25000.0)
    frames = torch.rand(N_FRAMES, 3, *HW, generator=torch.Generator().manual_seed(5)).to(DEV)
    em = DiffEntropyModel("gaussian")
    if name == "HNeRV_Boost":
        with torch.no_grad():
            model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    v1, wide, wide_g = io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.encode(model, em, args, frames, v1)
    budget = codec.encode(model, em, args, frames, wide, run=RUN, tables="empirical", wide=True)
    budget_g = codec.encode(model, em, args, frames, wide_g, run=RUN, wide=True)
    assert model.training                                  # (the mode is put back)
    _shared[name] = dict(v1=v1.getvalue(), wide=wide.getvalue(), wide_g=wide_g.getvalue(), budget=budget, budget_g=budget_g, model=model, em=em,
                         args=args, frames=frames)
    return _shared[name]


@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost"])
def test_device_encode_wide_writes_the_bytes_of_the_host_repack_where_the_narrow_kinds_refuse(name):
    from boosting_nerv_amd import codec, estream, wstream
    ref = _encoded(name)
    ws = wstream.read(ref["wide"])
    r0 = ws.tensors[0]
    assert 20000 <= r0.hi - r0.lo + 1 <= 30000 and r0.shift == 3 and all(r.shift == 0 for r in ws.tensors[1:] + ws.embeds)
    host, host_g = io.BytesIO(), io.BytesIO()
    budget = codec.repack(ref["v1"], host, RUN, tables="empirical", wide=True)
    assert ref["wide"][:4] == b"BNRW" and ref["wide"] == host.getvalue() and ref["budget"] == budget == wstream.info(ref["wide"]) == codec.info(ref["wide"])
    assert budget["total"] == 8 * len(ref["wide"]) == sum(budget[k] for k in estream.ITEMS) and budget["ans_run"] == RUN
    assert budget["n_wide_records"] == 1 and budget["max_shift"] == 3 and budget["n_embeds"] == (N_FRAMES if name == "HNeRV_Boost" else 0)
    assert codec.repack(ref["v1"], host_g, RUN, wide=True) == ref["budget_g"] and host_g.getvalue() == ref["wide_g"]
    assert ref["budget_g"]["n_table_records"] == 0
    print(f"{name}: BNRV {len(ref['v1'])} bytes, BNRW {len(ref['wide'])} bytes (empirical), {len(ref['wide_g'])} bytes (gaussian), run {RUN}; the wide "
          f"record: {r0.count} symbols on {r0.hi - r0.lo + 1} values, model {r0.model}")
    for tables_ in ("gaussian", "empirical"):              # today's raise sites stay
        with pytest.raises(NotImplementedError, match="4096"):
            codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], io.BytesIO(), run=RUN, tables=tables_)
    with pytest.raises(ValueError, match="run > 0"):
        codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], io.BytesIO(), wide=True)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost"])
def test_wide_file_decodes_to_the_frames_of_the_version_1_file(name, use_graph):
    from boosting_nerv_amd import codec
    ref = _encoded(name)
    a = codec.Decoder(io.BytesIO(ref["wide"]), DEV, use_graph=use_graph)
    b = codec.Decoder(io.BytesIO(ref["v1"]), DEV, use_graph=use_graph)
    assert (a.kind, b.kind) == ("wide", "cem") and len(a) == len(b) == N_FRAMES and a.frame_hw == b.frame_hw == HW
    for (ka, va), (kb, vb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    if name == "HNeRV_Boost":
        assert torch.equal(a.embeds, b.embeds)
    for i in (2, 0, 1, 3):
        assert torch.equal(a.decode_f32(i), b.decode_f32(i)), (name, i)
    for x, y in zip(a, b):                                 # the pipelined uint8 iterator
        assert np.array_equal(x, y)
    if not use_graph:                                      # the file under Gaussians alone holds the same model
        g = codec.Decoder(io.BytesIO(ref["wide_g"]), DEV, use_graph=False)
        assert all(torch.equal(va, vb) for va, vb in zip(g.model.state_dict().values(), b.model.state_dict().values()))


# ---------------------------------------------------------------------------------------------------------------------- command line
def _pack_ref(x):
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_cli_train_with_bitstream_wide_then_info_and_decode(tmp_path, monkeypatch, capsys):
    """train_nerv_compression --bitstream tiny.bnrw --bitstream_run 256 --bitstream_wide on the 4-frame recipe: the file is the new kind,
    the logged line is its budget, `codec info` adds up to 8 * size, `codec decode` writes the byte packing of Decoder.decode_f32."""
    from PIL import Image
    from boosting_nerv_amd import codec, estream, wstream
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "tiny.bnrw")
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
             "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 "
             "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
             "-e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
             "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1 "
             f"--bitstream {path} --bitstream_run 256 --bitstream_wide")
    seen = {}
    orig_eval = C.evaluate

    def spy(model, loader, rank, args, *a, **k):
        out = orig_eval(model, loader, rank, args, *a, **k)
        seen["args"] = args
        return out
    monkeypatch.setattr(C, "evaluate", spy)
    C.main(flags.split())
    size = os.path.getsize(path)
    assert open(path, "rb").read(4) == wstream.MAGIC
    budget = wstream.info(path)
    assert seen["args"].bitstream_budget == budget and budget["total"] == 8 * size and budget["ans_run"] == 256 and budget["n_embeds"] == 4
    assert budget["ans_tables"] == "gaussian" and budget["n_table_records"] == 0
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    line = [x for x in log.splitlines() if x.startswith("Bitstream ")]
    assert len(line) == 1 and line[0].rstrip() == f"Bitstream {path}: {codec.describe_wide(budget)}"
    capsys.readouterr()
    assert codec.main(["info", path]) == budget
    printed = capsys.readouterr().out
    assert f"{size} bytes = {8 * size} bits" in printed and sum(budget[k] for k in estream.ITEMS) == 8 * size
    out_dir = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(out_dir)]) == 4
    names = sorted(os.listdir(out_dir))
    assert names == [f"frame_{i:04d}.png" for i in range(4)]
    dec = codec.Decoder(path, DEV)
    assert dec.kind == "wide"
    for i, n in enumerate(names):
        img = Image.open(out_dir / n)
        assert img.size == (320, 180) and img.mode == "RGB"
        assert np.array_equal(np.asarray(img), _pack_ref(dec.decode_f32(i))[0].cpu().numpy())
