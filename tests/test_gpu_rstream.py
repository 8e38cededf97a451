"""The chunked CEM file on the GPU (``-m gpu``): the one-launch rANS decode + de-quantisation against the host decoder
of the same library, the chunked file against the version-1 file of the same model -- frame for frame, bit for bit -- and the command
line.  Valid streams only: damaged ones are the host suite's (tests/test_rstream_cpu.py)."""
import io
import os

import numpy as np
import pytest
import torch

from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 12, 63, 64, 65, 128, 4097)                   # at run 64: 4097 symbols are 65 runs -- a second block of one record
ALPHABETS = (2, 3, 256, 4096)


def _record(n, alphabet, rng, run, with_beta, offset):
    """One record: symbols on an alphabet of `alphabet` values, coded in runs on the host and decoded back by the host decoder (the
    oracle), and an output view `offset` elements into a 16-byte aligned NaN buffer with three guard elements behind it."""
    from boosting_nerv_amd.lib import entropy_model as em
    lo = int(rng.integers(-3000, 3000))
    hi = lo + alphabet - 1
    mean, std = lo + 0.45 * alphabet, max(0.2 * alphabet, 0.6)
    sym = np.clip(np.rint(rng.normal(mean, std, size=n)), lo, hi).astype(np.int32)
    sym[:2] = (lo, hi)[:n] if n >= 2 else sym[:2]        # both ends of the table
    words, run_words = em.ans_encode_gaussian_runs(sym, lo, hi, mean, std, run)
    host = em.ans_decode_gaussian_runs(words, run_words, n, lo, hi, mean, std, run)
    assert np.array_equal(host, sym)
    buf = torch.full((n + offset + 3,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    scale = float(np.float32(rng.uniform(1e-3, 0.05)))
    beta = float(np.float32(rng.normal())) if with_beta else None
    return dict(out=buf[offset:offset + n], buf=buf, offset=offset, host=host, words=words, scale=scale, beta=beta,
                item=(buf[offset:offset + n], scale, lo, hi, mean, std, run_words, beta))


def _check(records):
    for k, r in enumerate(records):
        want = torch.from_numpy(r["host"]).to(DEV).float() * torch.tensor(r["scale"], device=DEV)
        if r["beta"] is not None:
            want = want + torch.tensor(r["beta"], device=DEV)
        assert torch.equal(r["out"], want), (k, r["host"].size, (r["out"] != want).sum().item())
        o, n = r["offset"], r["host"].size
        assert torch.isnan(r["buf"][:o]).all().item() and torch.isnan(r["buf"][o + n:]).all().item(), k      # both sides untouched


def _launch(records, run):
    from boosting_nerv_amd import ops
    outs = ops.ans_dequant(np.concatenate([r["words"] for r in records]), [r["item"] for r in records], run)
    assert all(a.data_ptr() == r["out"].data_ptr() for a, r in zip(outs, records))


@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_ans_dequant_equals_the_host_decoder(offset, with_beta):
    """Every size on every alphabet in ONE launch at run 64, outputs `offset` elements into their buffers."""
    rng = np.random.default_rng(100 + offset)
    records = [_record(n, a, rng, 64, with_beta, offset) for n in SIZES for a in ALPHABETS]
    assert all(r["out"].data_ptr() % 16 == 4 * offset for r in records)
    _launch(records, 64)
    _check(records)


def test_ans_dequant_fifty_records_mixed_forms():
    """50 records in one call: every third carries a beta, the alignments cycle."""
    rng = np.random.default_rng(21)
    records = [_record(5 + 37 * i, ALPHABETS[i % 4], rng, 64, i % 3 == 0, i % 4) for i in range(50)]
    _launch(records, 64)
    _check(records)


def test_ans_dequant_long_runs_are_stored_in_rounds():
    """run 1024: a lane's run is decoded and stored in 16 rounds of 64 symbols; 4097 symbols are four full runs and one of a single symbol.
    The last record fills a block with 64 full runs of a 4096-symbol alphabet -- more words than the block stages in LDS, so its lanes
    refill from memory -- and leaves five symbols to a second block."""
    rng = np.random.default_rng(22)
    records = [_record(4097, a, rng, 1024, i % 2 == 1, i) for i, a in enumerate(ALPHABETS)] + [_record(1500, 256, rng, 1024, True, 1)]
    records.append(_record(64 * 1024 + 5, 4096, rng, 1024, False, 2))
    assert records[-1]["words"].size > 2 * 8192          # (the block stages 8192)
    _launch(records, 1024)
    _check(records)


def test_ans_dequant_refuses_what_it_cannot_do():
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(23)
    r = _record(130, 256, rng, 64, False, 0)
    out, scale, lo, hi, mean, std, run_words, beta = r["item"]
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.ans_dequant(r["words"], [r["item"]], 100)
    with pytest.raises(ValueError, match="run lengths"):
        ops.ans_dequant(r["words"], [(out, scale, lo, hi, mean, std, run_words[:-1], beta)], 64)
    with pytest.raises(ValueError, match="add up"):
        ops.ans_dequant(r["words"][:-1], [r["item"]], 64)
    with pytest.raises(ValueError, match="state words"):
        ops.ans_dequant(r["words"], [(out, scale, lo, hi, mean, std, np.array([1, int(run_words.sum()) - 3, 2], np.uint16), beta)], 64)
    with pytest.raises(ValueError, match="symbol range"):
        ops.ans_dequant(r["words"], [(out, scale, lo, lo + 4096, mean, std, run_words, beta)], 64)
    with pytest.raises(Exception, match="GPU tensor"):
        ops.ans_dequant(r["words"], [(out.cpu(), scale, lo, hi, mean, std, run_words, beta)], 64)
    assert torch.isnan(r["buf"]).all().item()             # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------- file against file
def _quant(a):
    a.__dict__.update(quant=True, quant_model_bit=8, quant_bias_bit=8, quant_embed_bit=8, per_channel_w=False, per_channel_b=False,
                      per_channel_e=False, quantizer_w="scale", quantizer_b="scale", quantizer_e="scalebeta", embed_entropy=True)
    return a


_CONFIGS = {"HNeRV_Boost": configs.tiny_hnerv_quant, "NeRV_Boost": lambda: _quant(configs.tiny_nerv()), "ENeRV_Boost": lambda: _quant(configs.tiny_enerv())}
N_FRAMES, HW, RUN = 4, (180, 320), 256
_shared = {}


def _encoded(name):
    """One tiny quantised model per architecture, built as tests/test_gpu_codec.py::_encoded builds it, encoded as the version-1 file (the
    default call and run=0) and as the chunked file (run=256); the compression model's own evaluation forward of every frame is computed
    once and never written."""
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
    frames = torch.rand(N_FRAMES, 3, *HW, generator=torch.Generator().manual_seed(5)).to(DEV)
    em = DiffEntropyModel("gaussian")
    if name == "HNeRV_Boost":                              # the embedding quantiser takes its range from the first embedding it sees, as in training
        with torch.no_grad():
            model.embed_quantizer.init_data(model.forward_encoder(frames[0:1]))
    today, v1, chunked = io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.encode(model, em, args, frames, today)
    budget1 = codec.encode(model, em, args, frames, v1, run=0)
    budget = codec.encode(model, em, args, frames, chunked, run=RUN)
    model.eval()
    want = []
    with torch.no_grad():
        assert model.cal_params_eval_fused(em) is True
        for i in range(N_FRAMES):
            norm_idx = torch.tensor([float(i + 1) / N_FRAMES], dtype=torch.float64, device=DEV)
            if name == "HNeRV_Boost":
                _, _, dequant_e = model.forward_embed_quant(model.forward_encoder(frames[i:i + 1]))
                out = model.forward_decoder(dequant_e, norm_idx)[0]
            else:
                out = model(norm_idx, norm_idx=norm_idx)[0]
            want.append(out.clone())
    _shared[name] = dict(today=today.getvalue(), v1=v1.getvalue(), chunked=chunked.getvalue(), budget1=budget1, budget=budget, want=want)
    return _shared[name]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost", "ENeRV_Boost"])
def test_chunked_file_decodes_to_the_frames_of_the_version_1_file(name, use_graph):
    from boosting_nerv_amd import codec
    ref = _encoded(name)
    a = codec.Decoder(io.BytesIO(ref["chunked"]), DEV, use_graph=use_graph)
    b = codec.Decoder(io.BytesIO(ref["v1"]), DEV, use_graph=use_graph)
    assert (a.kind, b.kind) == ("chunked", "cem") and len(a) == len(b) == N_FRAMES and a.frame_hw == b.frame_hw == HW
    for (ka, va), (kb, vb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    if name == "HNeRV_Boost":
        assert torch.equal(a.embeds, b.embeds)
    for i in (2, 0, 1, 3):
        got = a.decode_f32(i)
        assert torch.equal(got, b.decode_f32(i)) and torch.equal(got, ref["want"][i]), (name, i)
    for x, y in zip(a, b):                                 # the pipelined uint8 iterator
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost", "ENeRV_Boost"])
def test_encode_run_0_is_todays_file_and_the_chunked_file_holds_its_records(name):
    from boosting_nerv_amd import bitstream, codec, rstream
    from boosting_nerv_amd.lib.entropy_model import ans_decode_gaussian
    ref = _encoded(name)
    assert ref["v1"] == ref["today"] and ref["v1"][:4] == b"BNRV" and ref["budget1"] == bitstream.info(ref["v1"])
    assert ref["chunked"][:4] == b"BNRC" and ref["budget"] == rstream.info(ref["chunked"]) == codec.info(ref["chunked"])
    budget = ref["budget"]
    assert budget["total"] == 8 * len(ref["chunked"]) == sum(budget[k] for k in rstream.ITEMS) and budget["ans_run"] == RUN
    bs, rs = bitstream.read(ref["v1"]), rstream.read(ref["chunked"])
    assert rs.settings == dict(bs.settings, ans_run=RUN) and rs.embed_shape == bs.embed_shape
    assert len(rs.raw) == len(bs.raw) and all(np.array_equal(x, y) for x, y in zip(rs.raw, bs.raw))
    assert len(rs.tensors) == len(bs.tensors) and len(rs.embeds) == len(bs.embeds) == (N_FRAMES if name == "HNeRV_Boost" else 0)
    for k, (r, v) in enumerate(zip(rs.tensors + rs.embeds, bs.tensors + bs.embeds)):
        assert (r.count, r.lo, r.hi, r.scale, r.mean, r.std, r.beta) == (v.count, v.lo, v.hi, v.scale, v.mean, v.std, v.beta)
        assert np.array_equal(rstream.decode_record(rs, k), ans_decode_gaussian(v.words, v.count, v.lo, v.hi, float(v.mean), float(v.std))), k
    print(f"{name}: version 1 {len(ref['v1'])} bytes, chunked (run {RUN}) {len(ref['chunked'])} bytes; "
          f"{(budget['ans_words'] + budget['run_index'] - ref['budget1']['coded_words']) / budget['n_symbols']:.4f} bits per symbol over the single messages")


# ---------------------------------------------------------------------------------------------------------------------- command line
def _pack_ref(x):
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_cli_train_with_bitstream_run_then_info_and_decode(tmp_path, monkeypatch, capsys):
    """train_nerv_compression --bitstream tiny.bnrc --bitstream_run 256 on the 4-frame recipe: the file is the chunked kind, the logged
    line is its budget, `codec info` adds up to 8 * size, `codec decode` writes the byte packing of Decoder.decode_f32."""
    from PIL import Image
    from boosting_nerv_amd import codec, rstream
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "tiny.bnrc")
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
             "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 "
             "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
             "-e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
             "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1 "
             f"--bitstream {path} --bitstream_run 256")
    seen = {}
    orig_eval = C.evaluate

    def spy(model, loader, rank, args, *a, **k):
        out = orig_eval(model, loader, rank, args, *a, **k)
        seen["args"] = args
        return out
    monkeypatch.setattr(C, "evaluate", spy)
    C.main(flags.split())
    size = os.path.getsize(path)
    assert open(path, "rb").read(4) == rstream.MAGIC
    budget = rstream.info(path)
    assert seen["args"].bitstream_budget == budget and budget["total"] == 8 * size and budget["ans_run"] == 256 and budget["n_embeds"] == 4
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    line = [x for x in log.splitlines() if x.startswith("Bitstream ")]
    assert len(line) == 1 and f"{size} bytes = {8 * size} bits" in line[0] and f"ANS words {budget['ans_words']} " in line[0]
    capsys.readouterr()
    assert codec.main(["info", path]) == budget
    printed = capsys.readouterr().out
    assert f"{size} bytes = {8 * size} bits" in printed and sum(budget[k] for k in rstream.ITEMS) == 8 * size
    out_dir = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(out_dir)]) == 4
    names = sorted(os.listdir(out_dir))
    assert names == [f"frame_{i:04d}.png" for i in range(4)]
    dec = codec.Decoder(path, DEV)
    assert dec.kind == "chunked"
    for i, n in enumerate(names):
        img = Image.open(out_dir / n)
        assert img.size == (320, 180) and img.mode == "RGB"
        assert np.array_equal(np.asarray(img), _pack_ref(dec.decode_f32(i))[0].cpu().numpy())
