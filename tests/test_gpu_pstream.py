"""The temporal post-hoc model file on the GPU (``-m gpu``): the three new launches against numpy and the host coder, bit for
bit; the device encode path against the host path, byte for byte; Decoder against the .bnrq / .bnrz file of the same evaluation; and one
train_nerv_all --bitstream --bitstream_temporal run whose file decodes to the dumped PNGs."""
import glob
import io
import os

import numpy as np
import pytest
import torch

import hnerv_ref
import pstream_cases as PC
import qstream_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5
_shared = {}


def _rows(n, count, pad, shift, dtype=torch.uint8, fill=GUARD):
    """A [n, count] view with row pitch count + pad that starts `shift` elements into a buffer filled with `fill` -> (view, buffer)."""
    buf = torch.full((shift + n * (count + pad) + 16,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return torch.as_strided(buf, (n, count), (count + pad, 1), shift), buf


def _untouched(buf, view, rows=None):
    """Every element of `buf` outside the written rows of `view` still holds the fill value."""
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    n, count = view.shape
    first = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    for t in (range(n) if rows is None else rows):
        mask[first + t * view.stride(0):first + t * view.stride(0) + count] = False
    rest = buf[mask]
    return bool((torch.isnan(rest) if buf.dtype.is_floating_point else rest == GUARD).all().item())


# ---------------------------------------------------------------------------------------------------------------------- EmbedDeltaU8
@pytest.mark.parametrize("count", [1, 3, 15, 16, 17, 255, 256, 257, 2304, 2307])
def test_embed_delta_u8_is_exact(count):
    """d and both histograms equal numpy's for N in {1, 2, 5}: dense aligned rows; odd padded pitches (every row at another phase of the
    16-byte line) from a base one byte past a 16-byte line; nothing outside the rows of d is written, row 0 of d included."""
    from boosting_nerv_amd import ops, pstream
    rng = np.random.default_rng(count)
    for n in (1, 2, 5):
        q = rng.integers(0, 256, size=(n, count)).astype(np.uint8)
        q[n // 2] = rng.integers(0, 3, size=count)           # a skewed frame: many lanes on one bin
        want_d, want_h0, want_h1 = pstream.symbols(q)
        for qpad, dpad, shift in ((0, 0, 0), (5, 9, 1), (1, 0, 17)):
            qv, _ = _rows(n, count, qpad, shift)
            dv, dbuf = _rows(n, count, dpad, shift + (2 if dpad else 0))
            qv.copy_(torch.from_numpy(q))
            assert qv.data_ptr() % 16 == shift % 16
            job = ops.EmbedDeltaU8(qv, dv).launch().check()
            d, h0, h1 = job.host()
            assert np.array_equal(d[1:], want_d[1:]) and not d[0].any(), (n, count, qpad, dpad, shift)
            assert np.array_equal(h0, want_h0) and np.array_equal(h1, want_h1), (n, count, qpad, dpad, shift)
            assert _untouched(dbuf, dv, range(1, n)), (n, count, qpad, dpad, shift)
        d, h0, h1 = ops.EmbedDeltaU8(torch.from_numpy(q).to(DEV)).launch().host()      # the op's own buffer: one copy for all three
        assert np.array_equal(d, want_d) and np.array_equal(h0, want_h0) and np.array_equal(h1, want_h1)


def test_embed_delta_u8_more_than_one_block_per_frame_and_a_relaunch():
    from boosting_nerv_amd import ops, pstream
    rng = np.random.default_rng(7)
    q = rng.integers(0, 256, size=(3, 16 * 256 * 2 + 16 * 3 + 5)).astype(np.uint8)     # two blocks and a bit per frame, a tail of five
    job = ops.EmbedDeltaU8(torch.from_numpy(q).to(DEV))
    want = pstream.symbols(q)
    for _ in range(2):                                       # the entry point zeroes the histograms itself
        got = job.launch().host()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_embed_delta_u8_refuses_bad_tensors():
    from boosting_nerv_amd import ops
    q = torch.zeros(2, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.EmbedDeltaU8(q.int())
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.EmbedDeltaU8(q.t())
    with pytest.raises(ValueError, match="d is"):
        ops.EmbedDeltaU8(q, torch.zeros(2, 9, dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- HuffDecodeU8
def _decode_rows(sym_rows, lengths=None, shift=0, pad=0):
    """Code the rows (one item each) with the host coder, decode them with ONE ops.HuffDecodeU8 launch into rows `pad` apart that start
    `shift` bytes into a guarded buffer -> (device rows, buffer, words, run_bits, lengths)."""
    from boosting_nerv_amd import codec, ops, qstream
    from boosting_nerv_amd.lib.entropy_model import huff_decode, huff_encode
    n, count = len(sym_rows), sym_rows[0].size
    flat = np.concatenate(sym_rows)
    if lengths is None:
        lengths = codec.huffman_lengths(np.bincount(flat, minlength=256))
    words, run_bits = huff_encode(flat, [count] * n, lengths, qstream.RUN)
    assert np.array_equal(huff_decode(words, run_bits, [count] * n, lengths), flat)
    view, buf = _rows(n, count, pad, shift)
    per = qstream.n_runs(count)
    ops.HuffDecodeU8(words, lengths, [(view[t], run_bits[t * per:(t + 1) * per]) for t in range(n)]).launch().check()
    return view, buf, words, run_bits, lengths


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2304])
def test_huff_decode_u8_equals_the_host_decoder(count):
    rng = np.random.default_rng(count)
    rows = [np.rint(rng.normal(128, 12, size=count)).clip(0, 255).astype(np.uint8) for _ in range(3)]
    for shift, pad in ((0, 0), (1, 3), (2, 0), (3, 2)):      # rows that start at every byte phase of a dword
        view, buf, _, _, _ = _decode_rows(rows, shift=shift, pad=pad)
        assert np.array_equal(view.cpu().numpy(), np.stack(rows)), (count, shift, pad)
        assert _untouched(buf, view), (count, shift, pad)


def test_huff_decode_u8_code_lengths_above_the_table_bits_and_many_blocks():
    from boosting_nerv_amd import _lib as L
    q = Q.depth16_symbols()                                  # 65 535 symbols: 256 runs, four blocks; the rarest has a 16-bit code
    rows = list(q.reshape(5, -1))                            # five rows of 13 107 symbols: odd row starts, a short last run each
    assert rows[0].size % 2 == 1
    view, buf, _, _, lengths = _decode_rows(rows, shift=1, pad=1)
    assert lengths.max() >= 15 > L.HUFF_LUT_BITS
    assert np.array_equal(view.cpu().numpy(), np.stack(rows)) and _untouched(buf, view)


def test_huff_decode_u8_refuses_bad_items_before_any_launch():
    from boosting_nerv_amd import ops
    out = torch.zeros(300, dtype=torch.uint8, device=DEV)
    rb = np.array([100, 50], dtype=np.uint16)
    words, lengths = np.zeros(5, dtype=np.uint32), np.r_[np.full(256, 8), [0]].astype(np.uint8)
    with pytest.raises(ValueError, match="uint8 tensor"):
        ops.HuffDecodeU8(words, lengths, [(out.float(), rb)])
    with pytest.raises(ValueError, match="run lengths for"):
        ops.HuffDecodeU8(words, lengths, [(out, rb[:1])])
    with pytest.raises(ValueError, match="add up"):
        ops.HuffDecodeU8(words[:3], lengths, [(out, rb)])


def _embed_jobs(ps, held):
    """What codec.Decoder launches for the embedding section's strings of a read file."""
    from boosting_nerv_amd import ops, pstream
    e = ps.embeds
    jobs = []
    for kind, lengths, words in ((pstream.INTRA, e.lengths0, e.words0), (pstream.INTER, e.lengths1, e.words1)):
        rows = np.flatnonzero(e.pred == kind)
        if rows.size:
            jobs.append(ops.HuffDecodeU8(words, lengths, [(held[int(t)], e.run_bits[int(t)]) for t in rows]).launch())
    return jobs


def test_a_file_with_a_moved_run_boundary_raises_through_check():
    """One run length of an inter frame one bit longer, the next one bit shorter, the CRC recomputed: read() has nothing to refuse -- the
    lengths still add up -- and the lane of the second run starts one bit late.  It decodes its own symbol count from staged words and
    writes its own 256 bytes, whatever the bits are; the device error word makes ValueError."""
    from boosting_nerv_amd import pstream
    q = PC.walk_clip(8)
    blob, _, e = PC.file_of(q)
    good = pstream.read(blob)
    held = torch.full((8, PC.P), GUARD, dtype=torch.uint8, device=DEV)
    for job in _embed_jobs(good, held):
        job.check()
    assert np.array_equal(PC.chain(held.cpu().numpy(), e.pred), q)
    rb = e.run_bits.copy()
    rb[5, 0] += 1
    rb[5, 1] -= 1
    ps = pstream.read(PC.damaged(q, run_bits=rb))
    held2 = torch.full((8, PC.P), GUARD, dtype=torch.uint8, device=DEV)
    intra, inter = _embed_jobs(ps, held2)
    intra.check()
    with pytest.raises(ValueError, match="did not end on its recorded bit"):
        inter.check()
    rest = [t for t in range(8) if t != 5]
    assert torch.equal(held2[rest], held[rest])              # every other frame is whole


# ---------------------------------------------------------------------------------------------------------------------- EmbedChainDequantU8
def _preds(n):
    alt = (np.arange(n) % 2).astype(np.uint8)
    cases = {"all-intra": np.zeros(n, dtype=np.uint8), "all-inter": np.r_[0, np.ones(n - 1)].astype(np.uint8), "alternating": alt}
    for cut in (1, n - 1):
        if 0 < cut < n:
            p = np.r_[0, np.ones(n - 1)].astype(np.uint8)
            p[cut] = 0
            cases[f"cut-{cut}"] = p
    return cases


@pytest.mark.parametrize("flag", [PC.F32, PC.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65, 130])
def test_embed_chain_dequant_u8_equals_numpy(n, flag):
    """torch.equal to float32(min) + float32(scale) * float32(q) with q the numpy chain: every pred pattern, one pair for the whole tensor and
    grids reduced over axis 0, 1, 2 and 3 of the [N, 4, 3, 5] tensor; the symbols make every chain wrap mod 256."""
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(n)
    shape, count = (4, 3, 5), 60
    sym = rng.integers(0, 256, size=(n, count)).astype(np.uint8)
    sym_d = torch.from_numpy(sym).to(DEV)
    for name, pred in _preds(n).items():
        q = PC.chain(sym, pred)
        for axis in (None, 0, 1, 2, 3):
            lo, step, outer, red, inner = PC.grid(n, count, axis, flag, rng, shape)
            out = torch.full((n, count), float("nan"), device=DEV)
            ops.EmbedChainDequantU8(sym_d, pred, torch.from_numpy(lo).to(DEV), torch.from_numpy(step).to(DEV), red, inner, out).launch().check()
            want = torch.from_numpy(PC.restate(q, lo, step, outer, red, inner))
            assert torch.equal(out.cpu(), want), (n, name, axis, int((out.cpu() != want).sum()))


@pytest.mark.parametrize("count", [1, 3, 1027])
def test_embed_chain_dequant_u8_odd_rows_and_padded_pitches(count):
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(count)
    n = 5
    sym = rng.integers(0, 256, size=(n, count)).astype(np.uint8)
    pred = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    lo, step, outer, red, inner = PC.grid(n, count, 0, PC.F16, rng)
    want = torch.from_numpy(PC.restate(PC.chain(sym, pred), lo, step, outer, red, inner))
    for spad, opad, shift in ((0, 0, 0), (3, 1, 1), (2, 3, 2), (5, 2, 3)):
        sv, _ = _rows(n, count, spad, shift)
        ov, obuf = _rows(n, count, opad, shift, torch.float32, float("nan"))
        sv.copy_(torch.from_numpy(sym))
        ops.EmbedChainDequantU8(sv, pred, torch.from_numpy(lo).to(DEV), torch.from_numpy(step).to(DEV), red, inner, ov).launch()
        assert torch.equal(ov.cpu(), want) and _untouched(obuf, ov), (count, spad, opad, shift)


def test_embed_chain_dequant_u8_refuses_before_any_launch():
    from boosting_nerv_amd import ops
    sym = torch.zeros(3, 8, dtype=torch.uint8, device=DEV)
    out = torch.full((3, 8), float("nan"), device=DEV)
    lo = step = torch.ones(1, device=DEV)
    with pytest.raises(ValueError, match=r"frame 0 is predicted \(pred\[0\] = 1\)"):
        ops.EmbedChainDequantU8(sym, [1, 0, 0], lo, step, 24, 1, out)
    with pytest.raises(ValueError, match="values 0 \\| 1"):
        ops.EmbedChainDequantU8(sym, [0, 2, 0], lo, step, 24, 1, out)
    with pytest.raises(ValueError, match="slices"):
        ops.EmbedChainDequantU8(sym, [0, 1, 0], lo, step, 7, 1, out)
    with pytest.raises(ValueError, match="entries each"):
        ops.EmbedChainDequantU8(sym, [0, 1, 0], lo, step, 8, 1, out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item()


# ---------------------------------------------------------------------------------------------------------------------- encoder and decoder
N_FRAMES, HW = 4, (180, 320)


def _evaluation(sparse):
    """The tiny HNeRV model with seeded, perturbed weights (40 % of them zero for the sparse kind) and evaluate()'s steps for the quantised
    twin at -b 1, computed once: quant_model, the embeddings of the fp32 model quantised as one [N, C, h, w] tensor."""
    key = ("eval", sparse)
    if key in _shared:
        return _shared[key]
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import quant_tensor
    from boosting_nerv_amd.synth import SyntheticVideo
    args = hnerv_ref.tiny_args()
    args.__dict__.update(model="HNeRV", quant_model_bit=8, quant_embed_bit=6, crop_list="180_320", final_size=HW[0] * HW[1], full_data_length=N_FRAMES,
                         batchSize=1, bitstream_sparse=sparse)
    torch.manual_seed(3)
    model = T.build_model(args).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
                if sparse:
                    p.mul_((torch.rand_like(p) > 0.4).float())
    vid = SyntheticVideo(N_FRAMES, *HW)
    frames = torch.stack([vid.frame(i) for i in range(N_FRAMES)]).to(DEV)
    norms = [torch.tensor([float(i + 1) / N_FRAMES], dtype=torch.float64, device=DEV) for i in range(N_FRAMES)]
    with torch.no_grad():
        (plain, _), records = T.quant_model(model, args)
        plain.eval()
        embeds = [plain(frames[i:i + 1], None, norm_idx=norms[i])[1][0] for i in range(N_FRAMES)]
        quant_embed, _ = quant_tensor(torch.cat(embeds, 0), args.quant_embed_bit)
    _shared[key] = (model, args, records, quant_embed)
    return _shared[key]


def _walk_record(quant_embed):
    """The evaluation's embedding record with its codes replaced by a +-1 walk of the same shape: every later frame is inter, chains wrap."""
    q = quant_embed["quant"]
    rng = np.random.default_rng(11)
    walk = np.zeros((q.shape[0], q[0].numel()), dtype=np.uint8)
    walk[0] = rng.integers(0, 256, size=walk.shape[1])
    for t in range(1, q.shape[0]):
        walk[t] = walk[t - 1] + rng.integers(-1, 2, size=walk.shape[1]).astype(np.uint8)
    return dict(quant_embed, quant=torch.from_numpy(walk).reshape(q.shape).to(q.device))


def _files(sparse, walk):
    key = ("files", sparse, walk)
    if key not in _shared:
        from boosting_nerv_amd import codec
        model, args, records, quant_embed = _evaluation(sparse)
        rec = _walk_record(quant_embed) if walk else quant_embed
        plain, temporal = io.BytesIO(), io.BytesIO()
        codec.encode_posthoc(model, args, records, rec, plain)
        budget = codec.encode_posthoc(model, args, records, rec, temporal, temporal=True)
        _shared[key] = (plain.getvalue(), temporal.getvalue(), budget, rec)
    return _shared[key]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_device_records_and_their_cpu_copies_write_the_same_bytes(sparse):
    from boosting_nerv_amd import codec, pstream
    model, args, records, quant_embed = _evaluation(sparse)
    for walk in (False, True):
        _, blob, budget, rec = _files(sparse, walk)
        assert rec["quant"].is_cuda
        host = io.BytesIO()
        on_cpu = {k: v.cpu() for k, v in rec.items()}
        assert codec.encode_posthoc(model, args, records, on_cpu, host, temporal=True) == budget
        assert host.getvalue() == blob, (sparse, walk)
        assert budget["total"] == 8 * len(blob) and budget["tensor_kind"] == ("sparse" if sparse else "dense")
        q = rec["quant"].reshape(N_FRAMES, -1).cpu().numpy()
        assert budget["embed_section_bits"] <= pstream.all_intra_section_bits(q)
        assert np.array_equal(pstream.decode_embeds(pstream.read(blob)), q)
        if walk:
            assert budget["n_inter_frames"] == N_FRAMES - 1
        print(f"sparse={sparse} walk={walk}: {codec.describe_any(budget)}")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_decoder_equals_the_decoder_of_the_plain_file(sparse, use_graph):
    """Embeddings, every tensor and every frame of the .bnrp file are torch.equal to those of the .bnrq / .bnrz file of the same evaluation."""
    from boosting_nerv_amd import codec
    for walk in (False, True):
        plain, temporal, budget, _ = _files(sparse, walk)
        ref = codec.Decoder(io.BytesIO(plain), DEV, use_graph=use_graph)
        dec = codec.Decoder(io.BytesIO(temporal), DEV, use_graph=use_graph)
        assert ref.kind == ("sparse" if sparse else "posthoc") and dec.kind == "posthoc_temporal" and len(dec) == N_FRAMES and dec.frame_hw == HW
        assert dec.settings["embed_pred"] == "prev" and torch.equal(dec.embeds, ref.embeds)
        for (k, a), (_, b) in zip(dec.model.state_dict().items(), ref.model.state_dict().items()):
            assert torch.equal(a, b), k
        for i in (2, 0, 1, 3):
            assert torch.equal(dec.decode_f32(i), ref.decode_f32(i)), (sparse, walk, i)
            assert np.array_equal(dec.decode_u8(i), ref.decode_u8(i)), (sparse, walk, i)


# ---------------------------------------------------------------------------------------------------------------------- CLI
_RECIPE = ("--model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
           "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 --lr 0.001")


def test_temporal_flag_needs_a_file_and_a_model_with_embeddings():
    from boosting_nerv_amd import train_nerv_all as T
    with pytest.raises(ValueError, match="--bitstream_temporal: the temporal kind is what --bitstream FILE writes"):
        T.main("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV --crop_list 180_320 -e 1 --bitstream_temporal".split())
    with pytest.raises(ValueError, match="--bitstream_temporal: --model NeRV_Boost has no frame embeddings"):
        T.main("--outf t --data_path synthetic:4x180x320 --vid tiny --model NeRV_Boost --crop_list 180_320 -e 1 --bitstream t.bnrp --bitstream_temporal".split())


@pytest.mark.isolated
def test_cli_run_writes_a_temporal_file_that_decodes_to_the_dumped_images(tmp_path, monkeypatch):
    """The README's tiny recipe with --dump_images --bitstream t.bnrp --bitstream_temporal: `codec decode` gives the PNGs of
    visualize_model_quant byte for byte, eager and with the graph; the log's Huffman line is the one a run without the flag prints; --eval_only
    on the same checkpoint writes the .bnrq file of the same frames and, with --bitstream_sparse, the sparse temporal file of the same embeddings."""
    from PIL import Image
    from boosting_nerv_amd import codec, pstream
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    base = f"--data_path synthetic:4x180x320 --vid tiny {_RECIPE} --crop_list 180_320 --resize_list -1 --modelsize 0.05 --lower_width 6 -b 1 --eval_freq 1 -p 2 -e 2 --outf t"
    T.main((base + " --not_resume --dump_images --bitstream t.bnrp --bitstream_temporal").split())
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    path = str(tmp_path / "t.bnrp")
    budget = pstream.info(path)
    size = os.path.getsize(path)
    log = (out / "rank0.txt").read_text().splitlines()
    line = [x for x in log if x.startswith("Bitstream ")]
    assert len(line) == 1 and f"{size} bytes = {8 * size} bits" in line[0] and f"{budget['n_inter_frames']} as differences" in line[0]
    report = [x for x in log if "bits per parameter" in x]
    for use_graph in (False, True):
        dec = codec.Decoder(path, DEV, use_graph=use_graph)
        assert dec.kind == "posthoc_temporal" and len(dec) == 4
        for i in range(4):
            png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
            assert len(png) == 1, png
            assert np.array_equal(dec.decode_u8(i), np.asarray(Image.open(png[0]))), (use_graph, i)
    frames = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(frames)]) == 4 and codec.main(["info", path]) == budget
    for i in range(4):
        png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
        assert np.array_equal(np.asarray(Image.open(frames / f"frame_{i:04d}.png")), np.asarray(Image.open(png[0]))), i
    # the same checkpoint as a plain file: the same report line, the same frames
    T.main((base + " --eval_only --bitstream t.bnrq").split())
    log = (out / "rank0.txt").read_text().splitlines()
    assert [x for x in log if "bits per parameter" in x][-1] == report[-1]
    plain = codec.Decoder(str(tmp_path / "t.bnrq"), DEV)
    assert all(np.array_equal(plain.decode_u8(i), dec.decode_u8(i)) for i in range(4)) and torch.equal(plain.embeds, dec.embeds)
    dense = codec.info(str(tmp_path / "t.bnrq"))
    assert dense["n_symbols"] == budget["n_symbols"] + budget["n_embed_symbols"]
    # and with --bitstream_sparse: the two flags combine
    T.main((base + " --eval_only --bitstream s.bnrp --bitstream_sparse --bitstream_temporal").split())
    both = codec.info(str(tmp_path / "s.bnrp"))
    assert both["tensor_kind"] == "sparse" and "zero_parse" in both and both["n_inter_frames"] == budget["n_inter_frames"]
    assert both["embed_symbol_bits"] == budget["embed_symbol_bits"]
    a = codec.Decoder(str(tmp_path / "s.bnrp"), DEV)
    assert a.kind == "posthoc_temporal" and torch.equal(a.embeds, dec.embeds)
    print(f".bnrp {budget['bytes']} bytes ({budget['n_inter_frames']} inter frames), .bnrq {dense['bytes']}; sparse .bnrp {both['bytes']}")
