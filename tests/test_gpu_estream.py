"""The chunked CEM file with per-record tables on the GPU (``-m gpu``): the histogram kernel against np.bincount, the
device encoder against the host coder of the same library bit for bit, the file codec.encode(..., tables="empirical") writes against the
host repack of the version-1 file of the same model, its decode against the version-1 decode frame for frame, and the command line."""
import io
import os

import numpy as np
import pytest
import torch

from oracle import configs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOTAL = 1 << 24


def _dev(sym):
    """int32 symbols on the device, starting one element past a 16-byte boundary."""
    buf = torch.zeros(sym.size + 1, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = torch.from_numpy(sym)
    out = buf[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---------------------------------------------------------------------------------------------------------------------- histogram
def test_sym_hist_equals_bincount():
    """Every size on every alphabet, a 12-element item and one of three slices, in ONE launch; every tensor one element off 16 bytes."""
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(40)
    host = []
    for n in (1, 63, 64, 65, 4097):
        for a in (2, 255, 4096):
            lo = int(rng.integers(-3000, 3000))
            host.append((rng.integers(lo, lo + a, size=n).astype(np.int32), lo, a))
    host.insert(3, (rng.integers(-5, 2, size=12).astype(np.int32), -5, 7))
    big = np.clip(np.rint(rng.laplace(0.0, 40.0, size=2 * L.HIST_SLICE + 777)), -2048, 2047).astype(np.int32)
    big[:2] = (-2048, 2047)
    host.insert(4, (big, -2048, 4096))
    got = ops.sym_hist([(_dev(s), lo, a) for s, lo, a in host])
    assert len(got) == len(host)
    for k, ((s, lo, a), g) in enumerate(zip(host, got)):
        assert g.dtype == np.uint32 and g.size == a and np.array_equal(g, np.bincount(s - lo, minlength=a)), (k, s.size, a)
    # the object is relaunchable: the counts are zeroed by every launch
    job = ops.SymHist([(_dev(host[4][0]), -2048, 4096)])
    job.launch().launch().check()
    assert np.array_equal(job.host()[0], np.bincount(big + 2048, minlength=4096))


def test_sym_hist_flags_a_symbol_outside_its_range_and_does_not_count_it():
    from boosting_nerv_amd import ops
    sym = np.array([0, 1, 2, 9, -1, 2], np.int32)
    job = ops.SymHist([(_dev(sym), 0, 3), (_dev(np.array([4, 4], np.int32)), 4, 2)]).launch()
    with pytest.raises(ValueError, match="outside"):
        job.check()
    assert [c.tolist() for c in job.host()] == [[1, 1, 2], [2, 0]]
    with pytest.raises(ValueError, match="alphabet"):
        ops.SymHist([(_dev(sym), 0, 4097)])
    with pytest.raises(ValueError, match="int32"):
        ops.SymHist([(_dev(sym).float(), 0, 3)])


# ---------------------------------------------------------------------------------------------------------------------- encoder
def _counts_cdf(sym, lo, a):
    from boosting_nerv_amd.lib import entropy_model as em
    return em.ans_counts_cdf(np.bincount(sym - lo, minlength=a))


def _encoder_cases(run, rng):
    """[(symbols, lo, cdf)] for one launch at `run`: a record of several blocks with a short last run, n = 1, exactly one run, one run and a
    symbol, the dominant-symbol table, the flat 4096-symbol table, a whole run of a one-slot symbol, a Gaussian table."""
    from boosting_nerv_amd.lib import entropy_model as em
    cases = []
    n = 64 * run + run // 2 + 3 if run <= 256 else 5 * run + 17          # (at run 64 and 256: a second block of the record)
    sym = np.clip(np.rint(rng.laplace(0.0, 6.0, size=n)), -60, 60).astype(np.int32)
    cases.append((sym, -60, _counts_cdf(sym, -60, 121)))
    for n in (1, run, run + 1):
        sym = rng.integers(10, 14, size=n).astype(np.int32)
        cases.append((sym, 10, _counts_cdf(sym, 10, 4)))
    dominant = em.ans_counts_cdf(np.array([1_000_000 - 1, 1], np.uint32))
    cases.append((np.zeros(3 * run, np.int32), 0, dominant))             # every run: its two state words
    one_slot = em.ans_counts_cdf(np.array([1_000_000, 0], np.uint32))
    assert one_slot[2] - one_slot[1] == 1
    cases.append((np.ones(run, np.int32), 0, one_slot))                  # the one-slot symbol for a whole run: 24 bits each
    flat = em.ans_counts_cdf(np.ones(4096, np.uint32))
    cases.append((rng.integers(-2048, 2048, size=2 * run + 5).astype(np.int32), -2048, flat))
    sym = np.clip(np.rint(rng.normal(3.0, 11.0, size=1000)), -40, 40).astype(np.int32)
    cases.append((sym, -40, em.ans_gaussian_cdf(-40, 40, 3.0, 11.0)))
    return cases


@pytest.mark.parametrize("run", [64, 256, 4096])
def test_ans_encode_runs_equals_the_host_coder_bit_for_bit(run):
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.lib import entropy_model as em
    cases = _encoder_cases(run, np.random.default_rng(run))
    want = [em.ans_encode_table_runs(s, lo, cdf, run) for s, lo, cdf in cases]
    assert want[4][1].tolist() == [2, 2, 2] and not want[4][0].any() and want[5][1].tolist() == [run * 24 // 32]
    enc = ops.AnsEncodeRuns([(_dev(s), lo, cdf) for s, lo, cdf in cases], run).launch().check()
    words, run_words = enc.result()
    assert words.dtype == np.uint32 and len(run_words) == len(cases)
    for k, ((w, rw), got) in enumerate(zip(want, run_words)):
        assert got.dtype == np.uint16 and np.array_equal(got, rw), (k, cases[k][0].size)
    assert np.array_equal(words, np.concatenate([w for w, _ in want]))
    # a chosen subset, in another order: the runs of those items alone
    words, run_words = enc.result([6, 0, 2])
    assert np.array_equal(words, np.concatenate([want[k][0] for k in (6, 0, 2)])) and all(np.array_equal(a, want[k][1]) for a, k in zip(run_words, (6, 0, 2)))
    # and what was encoded decodes on the device under the same tables
    outs = [torch.full((s.size + 2,), float("nan"), device=DEV) for s, _, _ in cases]
    ops.ans_dequant_tables(np.concatenate([w for w, _ in want]),
                           [(o[1:-1], 0.5, lo, cdf, rw, None) for o, (s, lo, cdf), (_, rw) in zip(outs, cases, want)], run)
    for o, (s, _, _) in zip(outs, cases):
        assert torch.equal(o[1:-1], torch.from_numpy(s).to(DEV).float() * 0.5) and torch.isnan(o[0]).item() and torch.isnan(o[-1]).item()


def test_ans_encode_runs_flags_a_symbol_outside_its_table():
    """An error flag, not a fault: the lane stops writing, check() raises, the other item's runs are what the host codes."""
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.lib import entropy_model as em
    rng = np.random.default_rng(41)
    good = rng.integers(0, 4, size=300).astype(np.int32)
    bad = good.copy()
    bad[130] = 4
    cdf = _counts_cdf(good, 0, 4)
    enc = ops.AnsEncodeRuns([(_dev(bad), 0, cdf), (_dev(good), 0, cdf)], 64).launch()
    with pytest.raises(ValueError, match="outside its table"):
        enc.check()
    with pytest.raises(ValueError, match="outside its table"):
        enc.result()
    rw = enc.run_words()
    want = em.ans_encode_table_runs(good, 0, cdf, 64)[1]
    assert rw[0][2] == 0 and np.array_equal(np.delete(rw[0], 2), np.delete(want, 2)) and np.array_equal(rw[1], want)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.AnsEncodeRuns([(_dev(good), 0, cdf)], 100)
    with pytest.raises(ValueError, match="rise strictly"):
        ops.AnsEncodeRuns([(_dev(good), 0, np.array([0, 5, 5, 9, TOTAL], np.uint32))], 64)
    with pytest.raises(Exception, match="GPU tensor"):
        ops.AnsEncodeRuns([(torch.from_numpy(good), 0, cdf)], 64)


# ---------------------------------------------------------------------------------------------------------------------- file against file
def _quant(a):
    a.__dict__.update(quant=True, quant_model_bit=8, quant_bias_bit=8, quant_embed_bit=8, per_channel_w=False, per_channel_b=False,
                      per_channel_e=False, quantizer_w="scale", quantizer_b="scale", quantizer_e="scalebeta", embed_entropy=True)
    return a


_CONFIGS = {"HNeRV_Boost": configs.tiny_hnerv_quant, "NeRV_Boost": lambda: _quant(configs.tiny_nerv()), "ENeRV_Boost": lambda: _quant(configs.tiny_enerv())}
N_FRAMES, HW, RUN = 4, (180, 320), 256
_shared = {}


def _encoded(name):
    """One tiny quantised model per architecture, built as tests/test_gpu_rstream.py::_encoded builds it: its version-1 file, its chunked
    file and the file with per-record tables, the last coded on the device."""
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
    v1, chunked, emp = io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.encode(model, em, args, frames, v1)
    codec.encode(model, em, args, frames, chunked, run=RUN)
    budget = codec.encode(model, em, args, frames, emp, run=RUN, tables="empirical")
    assert model.training                                  # (the mode is put back)
    _shared[name] = dict(v1=v1.getvalue(), chunked=chunked.getvalue(), emp=emp.getvalue(), budget=budget, model=model, em=em, args=args, frames=frames)
    return _shared[name]


def _size_condition(budget, bnrc):
    """Words, tables and side values of a BNRE budget take no more than those of the BNRC file of the same run, plus the model byte of every
    record; -> the record count."""
    from boosting_nerv_amd import rstream
    c = rstream.info(bnrc)
    n_rec = budget["n_tensors"] + budget["n_embeds"]
    assert budget["ans_run"] == c["ans_run"] and budget["n_symbols"] == c["n_symbols"] and n_rec == c["n_tensors"] + c["n_embeds"]
    assert budget["ans_words"] + budget["tables"] + budget["tensor_side"] + budget["embed_side"] <= c["ans_words"] + c["tensor_side"] + c["embed_side"] + 8 * n_rec
    return n_rec


@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost"])
def test_device_encode_follows_the_unfused_evaluation_pass(name, monkeypatch):
    """BNERV_CEM_EVAL_FUSED=0: evaluate() and the version-1 file take every tensor's moments from the tensor-by-tensor loop; the device path
    takes the same ones, so its file is still the host repack of that version-1 file."""
    from boosting_nerv_amd import codec
    ref = _encoded(name)
    monkeypatch.setenv("BNERV_CEM_EVAL_FUSED", "0")
    v1, chunked, emp, host = io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO()
    codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], v1)
    codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], chunked, run=RUN)
    budget = codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], emp, run=RUN, tables="empirical")
    assert codec.repack(v1.getvalue(), host, RUN, tables="empirical") == budget and emp.getvalue() == host.getvalue()
    _size_condition(budget, chunked.getvalue())
    print(f"{name}, unfused: the version-1 file {'equals' if v1.getvalue() == ref['v1'] else 'differs from'} the fused pass's")


@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost", "ENeRV_Boost"])
def test_device_encode_writes_the_bytes_of_the_host_repack(name):
    from boosting_nerv_amd import codec, estream
    ref = _encoded(name)
    host = io.BytesIO()
    budget = codec.repack(ref["v1"], host, RUN, tables="empirical")
    assert ref["emp"][:4] == b"BNRE" and ref["emp"] == host.getvalue() and ref["budget"] == budget == estream.info(ref["emp"]) == codec.info(ref["emp"])
    assert budget["total"] == 8 * len(ref["emp"]) == sum(budget[k] for k in estream.ITEMS) and budget["ans_run"] == RUN
    assert budget["n_embeds"] == (N_FRAMES if name == "HNeRV_Boost" else 0)
    n_rec = _size_condition(budget, ref["chunked"])
    print(f"{name}: BNRV {len(ref['v1'])} bytes, BNRC {len(ref['chunked'])} bytes, BNRE {len(ref['emp'])} bytes (run {RUN}); "
          f"{budget['n_table_records']} of {n_rec} records took a table")
    with pytest.raises(ValueError, match="run > 0"):
        codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], io.BytesIO(), tables="empirical")
    with pytest.raises(ValueError, match="tables"):
        codec.encode(ref["model"], ref["em"], ref["args"], ref["frames"], io.BytesIO(), run=RUN, tables="laplace")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["HNeRV_Boost", "NeRV_Boost", "ENeRV_Boost"])
def test_file_with_tables_decodes_to_the_frames_of_the_version_1_file(name, use_graph):
    from boosting_nerv_amd import codec
    ref = _encoded(name)
    a = codec.Decoder(io.BytesIO(ref["emp"]), DEV, use_graph=use_graph)
    b = codec.Decoder(io.BytesIO(ref["v1"]), DEV, use_graph=use_graph)
    assert (a.kind, b.kind) == ("empirical", "cem") and len(a) == len(b) == N_FRAMES and a.frame_hw == b.frame_hw == HW
    for (ka, va), (kb, vb) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    if name == "HNeRV_Boost":
        assert torch.equal(a.embeds, b.embeds)
    for i in (2, 0, 1, 3):
        assert torch.equal(a.decode_f32(i), b.decode_f32(i)), (name, i)
    for x, y in zip(a, b):                                 # the pipelined uint8 iterator
        assert np.array_equal(x, y)


def test_a_flipped_payload_byte_raises_at_the_crc():
    from boosting_nerv_amd import codec
    blob = bytearray(_encoded("NeRV_Boost")["emp"])
    blob[len(blob) // 2] ^= 0x04
    with pytest.raises(ValueError, match="CRC"):
        codec.Decoder(io.BytesIO(bytes(blob)), DEV)


# ---------------------------------------------------------------------------------------------------------------------- command line
def _pack_ref(x):
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_cli_train_with_bitstream_tables_empirical_then_info_and_decode(tmp_path, monkeypatch, capsys):
    """train_nerv_compression --bitstream tiny.bnre --bitstream_run 256 --bitstream_tables empirical on the 4-frame recipe: the file is the
    new kind, the logged line is its budget, `codec info` adds up to 8 * size, `codec decode` writes the byte packing of Decoder.decode_f32."""
    from PIL import Image
    from boosting_nerv_amd import codec, estream
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "tiny.bnre")
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan "
             "--conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 "
             "--enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 "
             "-e 1 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 "
             "--quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1 "
             f"--bitstream {path} --bitstream_run 256 --bitstream_tables empirical")
    seen = {}
    orig_eval = C.evaluate

    def spy(model, loader, rank, args, *a, **k):
        out = orig_eval(model, loader, rank, args, *a, **k)
        seen["args"] = args
        if k.get("write_bitstream"):                       # the chunked file of the same evaluation, for the size condition
            buf = io.BytesIO()
            codec.encode(model, k["entropy_model"], args, loader, buf, run=256)
            seen["bnrc"] = buf.getvalue()
        return out
    monkeypatch.setattr(C, "evaluate", spy)
    C.main(flags.split())
    size = os.path.getsize(path)
    assert open(path, "rb").read(4) == estream.MAGIC
    budget = estream.info(path)
    assert seen["args"].bitstream_budget == budget and budget["total"] == 8 * size and budget["ans_run"] == 256 and budget["n_embeds"] == 4
    _size_condition(budget, seen["bnrc"])
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    line = [x for x in log.splitlines() if x.startswith("Bitstream ")]
    assert len(line) == 1 and line[0].rstrip() == f"Bitstream {path}: {codec.describe_empirical(budget)}"
    capsys.readouterr()
    assert codec.main(["info", path]) == budget
    printed = capsys.readouterr().out
    assert f"{size} bytes = {8 * size} bits" in printed and sum(budget[k] for k in estream.ITEMS) == 8 * size
    out_dir = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(out_dir)]) == 4
    names = sorted(os.listdir(out_dir))
    assert names == [f"frame_{i:04d}.png" for i in range(4)]
    dec = codec.Decoder(path, DEV)
    assert dec.kind == "empirical"
    for i, n in enumerate(names):
        img = Image.open(out_dir / n)
        assert img.size == (320, 180) and img.mode == "RGB"
        assert np.array_equal(np.asarray(img), _pack_ref(dec.decode_f32(i))[0].cpu().numpy())
