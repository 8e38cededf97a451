"""The sparse post-hoc quantised model's file on the GPU (``-m gpu``): the decode kernel against the host coder and the
numpy restatement, bit for bit; the device error word; and train_nerv_all --bitstream --bitstream_sparse runs whose file decodes to the
dumped PNGs with every pruned weight exactly zero."""
import glob
import os

import numpy as np
import pytest
import torch

import qstream_cases as Q
import zstream_cases as Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _items(records, split, offset=False):
    items, bufs = [], []
    for (q, keep, lo, step, outer, red, inner, flag), rb in zip(records, split):
        buf = torch.full((q.size + 2 if offset else q.size,), float("nan"), device=DEV)
        out = buf[1:1 + q.size] if offset else buf
        assert out.data_ptr() % 16 == (4 if offset else 0)
        items.append((out, torch.from_numpy(lo).to(DEV), torch.from_numpy(step).to(DEV), red, inner, rb))
        bufs.append(buf)
    return items, bufs


def _run(records, offset=False, parse=None, lengths=None):
    """Code the host records, decode them with ONE ops.huffz_dequant launch, return the outputs (and their guard elements)."""
    from boosting_nerv_amd import ops
    words, lengths, split, parse = Z.stream(records, parse, lengths)
    items, bufs = _items(records, split, offset)
    ops.huffz_dequant(words, lengths, items)
    return [it[0] for it in items], bufs, lengths, (words, split, parse)


def _check(records, outs, coded=None):
    """Every output is the restatement of the record, bit for bit (a zero is +0.0); with `coded`, also of what the host decoder makes of
    the coded words."""
    for k, (rec, out) in enumerate(zip(records, outs)):
        want = Z.restate(*rec[:7])
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (k, rec[4:], int((got != want).sum()))
    if coded is not None:
        from boosting_nerv_amd.lib.entropy_model import huffz_decode
        words, lengths, split = coded
        sym, keep = huffz_decode(words, np.concatenate(split), [r[0].size for r in records], lengths)
        at = 0
        for rec, out in zip(records, outs):
            n = rec[0].size
            assert out.cpu().numpy().tobytes() == Z.restate(sym[at:at + n], keep[at:at + n], *rec[2:7]).tobytes()
            at += n


# ---------------------------------------------------------------------------------------------------------------------- kernel against host
@pytest.mark.parametrize("parse", Z.PARSES)
def test_kernel_equals_rebuilt_on_the_five_pruned_records(parse):
    five = Z.five_sparse_records(0.4)
    records = [r for r, _, _ in five]
    outs, _, lengths, (words, split, _) = _run(records, parse=parse)
    _check(records, outs, (words, lengths, split))
    for k, ((_, rebuilt, t), out) in enumerate(zip(five, outs)):
        assert out.cpu().numpy().tobytes() == rebuilt.tobytes(), k
        assert not out.cpu()[t.reshape(-1) == 0].any()


@pytest.mark.parametrize("parse", Z.PARSES)
def test_kernel_hand_built_grids_both_dtypes(parse):
    rng = np.random.default_rng(21)
    records = [Z.hand_record(g, flag, rng, keep) for flag in (Z.F32, Z.F16) for g, keep in (((3, 5, 7), 0.5), ((2, 300, 3), 0.1), ((1, 9, 40), 0.9), ((7, 1, 1), 0.5), (513, 0.3))]
    outs, _, lengths, (words, split, _) = _run(records, parse=parse)
    _check(records, outs, (words, lengths, split))


@pytest.mark.parametrize("parse", Z.PARSES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 64 * 256 - 1, 64 * 256 + 1])
def test_kernel_element_counts(n, parse):
    rng = np.random.default_rng(n)
    gauss = np.rint(rng.normal(120, 25, size=n)).clip(0, 255).astype(np.uint8)
    for keep in (0.6, 0.05):                                # (at n = 1: one kept element, then one zero)
        records = [Z.hand_record(n, Z.F32, rng, rng.random(n) < keep if n > 1 else [keep > 0.5], gauss)]
        outs, _, _, _ = _run(records, parse=parse)
        _check(records, outs)


def test_kernel_thirty_small_items_share_a_block_and_an_item_straddles_blocks():
    rng = np.random.default_rng(22)
    records = [Z.hand_record(3, Z.F16 if k % 2 else Z.F32, rng, 0.5) for k in range(30)]
    records += [Z.hand_record((4, 640, 1), Z.F16, rng, 0.6), Z.hand_record((1, 100, 256), Z.F16, rng, 0.2)]      # runs 30..39, then 40..139: over the 64-run block edge
    for parse in Z.PARSES:
        outs, _, _, _ = _run(records, parse=parse)
        _check(records, outs)


def test_kernel_outputs_four_bytes_off_a_sixteen_byte_boundary():
    rng = np.random.default_rng(23)
    records = [Z.hand_record(n, Z.F32, rng, 0.5) for n in (5, 256, 1000)] + [Z.hand_record((3, 50, 4), Z.F16, rng, 0.5)]
    outs, bufs, _, _ = _run(records, offset=True)
    _check(records, outs)
    for buf in bufs:                                        # the elements around every view were not touched
        assert torch.isnan(buf[0]).item() and torch.isnan(buf[-1]).item()


@pytest.mark.parametrize("parse", Z.PARSES)
def test_kernel_an_all_zero_record_and_a_record_without_a_zero(parse):
    rng = np.random.default_rng(27)
    records = [Z.hand_record((2, 450, 1), Z.F16, rng, np.zeros(900, dtype=bool)), Z.hand_record(900, Z.F32, rng, np.ones(900, dtype=bool)),
               Z.hand_record(1, Z.F32, rng, [False]), Z.hand_record(700, Z.F32, rng, np.arange(700) % 2 == 0)]
    outs, _, lengths, (words, split, _) = _run(records, parse=parse)
    if parse == "runs":                                     # one leaf per whole run of zeros
        code = int(lengths[Z.ZERO + 8])
        assert split[0][:3].tolist() == [code] * 3
    _check(records, outs, (words, lengths, split))
    assert not outs[0].any().item() and not torch.signbit(outs[0]).any().item()


def test_kernel_code_lengths_above_the_table_bits():
    from boosting_nerv_amd import _lib as L
    rng = np.random.default_rng(24)
    q = Q.depth16_symbols()
    keep = rng.random(q.size) < 0.7
    keep[q != 46] = True                                    # zeros among the most frequent symbol only: the rare ones keep their 2^k counts
    deep = [Z.hand_record(q.size, Z.F32, rng, keep, q)]
    for parse in Z.PARSES:
        outs, _, lengths, (words, split, _) = _run(deep, parse=parse)
        assert lengths.max() >= 15 > L.HUFF_LUT_BITS and lengths[Z.ZERO:Z.LEAVES - 1].any()      # codes past the first-level table: the canonical search
        _check(deep, outs, (words, lengths, split))
    rare = [Z.hand_record(q.size, Z.F32, rng, q != 1, q)]   # and a zero-run leaf that is itself the rarest: a long code for a zero
    outs, _, lengths, _ = _run(rare, parse="single")
    assert lengths[Z.ZERO] > L.HUFF_LUT_BITS
    _check(rare, outs)


def test_kernel_reads_from_memory_when_a_block_of_runs_outgrows_its_lds_span():
    """A valid but wasteful code -- lengths 1, 2, ..., 20 for the data leaves 0..19, 21 for one zero and for EOF -- and data made of its 17- to
    20-bit symbols with a few zeros: 64 full runs hold more than the 8192 words a block stages in LDS, so the first block takes the path that
    fetches its words from memory; the short last block stages."""
    lengths = np.zeros(Z.LEAVES, dtype=np.uint8)
    lengths[:20] = np.arange(1, 21)
    lengths[Z.ZERO] = lengths[Z.LEAVES - 1] = 21
    rng = np.random.default_rng(26)
    n = 70 * 256 + 9
    rec = Z.hand_record((1, n, 1), Z.F16, rng, rng.random(n) < 0.97, rng.integers(16, 20, size=n).astype(np.uint8))
    outs, _, _, (words, split, _) = _run([rec], parse="single", lengths=lengths)
    assert int(split[0][:64].sum(dtype=np.int64)) > 32 * 8192 and int(split[0][64:].sum(dtype=np.int64)) < 32 * 8000
    _check([rec], outs, (words, lengths, split))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_error_word_for_a_descriptor_shorter_than_its_bits():
    """Item 1 was coded with 300 elements and is described with 290: the lane of its second run reaches its element count (or clamps a zero
    run at it) before its recorded bit.  The device error word makes ValueError; the other items -- and nothing past the 290 elements -- are
    written as usual."""
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(28)
    records = [Z.hand_record(700, Z.F32, rng, 0.5), Z.hand_record(300, Z.F32, rng, 0.5), Z.hand_record((2, 200, 2), Z.F16, rng, 0.5)]
    words, lengths, split, _ = Z.stream(records)
    items, bufs = _items(records, split)
    guard = torch.full((300,), float("nan"), device=DEV)
    items[1] = (guard[:290], items[1][1], items[1][2], 290, 1, items[1][5])
    with pytest.raises(ValueError, match="did not end on its recorded bit"):
        ops.huffz_dequant(words, lengths, items)
    _check([records[0], records[2]], [items[0][0], items[2][0]])
    assert torch.isnan(guard[290:]).all().item()
    want = Z.restate(*records[1][:7])
    assert guard[:256].cpu().numpy().tobytes() == want[:256].tobytes()       # its first run is whole


def test_huffz_dequant_refuses_bad_items_before_any_launch():
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(25)
    rec = Z.hand_record(300, Z.F32, rng, 0.5)
    words, lengths, split, _ = Z.stream([rec])
    out, lo, step = torch.full((300,), float("nan"), device=DEV), torch.from_numpy(rec[2]).to(DEV), torch.from_numpy(rec[3]).to(DEV)
    with pytest.raises(ValueError, match="run lengths for"):
        ops.huffz_dequant(words, lengths, [(out, lo, step, 300, 1, split[0][:1])])
    with pytest.raises(ValueError, match="slices"):
        ops.huffz_dequant(words, lengths, [(out, lo, step, 7, 1, split[0])])
    with pytest.raises(ValueError, match="fp32 tensor"):
        ops.huffz_dequant(words, lengths, [(out.double(), lo, step, 300, 1, split[0])])
    with pytest.raises(ValueError, match="add up"):
        ops.huffz_dequant(words[:-1], lengths, [(out, lo, step, 300, 1, split[0])])
    with pytest.raises(ValueError, match="runs of 256"):     # wrong R
        ops.huffz_dequant(words, lengths, [(out, lo, step, 300, 1, split[0])], run=128)
    with pytest.raises(ValueError, match="need 266 code lengths"):
        ops.huffz_dequant(words, lengths[:257], [(out, lo, step, 300, 1, split[0])])
    bad = lengths.copy()
    bad[np.flatnonzero(lengths)[0]] += 1                     # an incomplete code
    with pytest.raises(L.BnervError, match="Kraft"):
        ops.huffz_dequant(words, bad, [(out, lo, step, 300, 1, split[0])])
    # the entry point itself: null and misaligned device pointers
    job = ops.HuffzDequant(words, lengths, [(out, lo, step, 300, 1, split[0])])
    lib, ln = L.load(), job.lengths.ctypes.data
    args = [L.stream(), L.ptr(job.words), job.n_words, L.ptr(job.runs), job.n_runs, L.ptr(job.items), job.n_items, ln, 256, L.ptr(job.err)]
    for k in (1, 3, 5, 9):
        broken = list(args)
        broken[k] = None
        assert lib.bnerv_huffz_dequant(*broken) == -1
    for k, what in ((1, b"4-byte"), (3, b"8-byte"), (5, b"8-byte"), (9, b"4-byte")):
        broken = list(args)
        broken[k] = C.c_void_p(args[k].value + 2)
        assert lib.bnerv_huffz_dequant(*broken) == -1 and what in lib.bnerv_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item() and int(job.err.item()) == 0      # nothing was launched


def test_sparse_flag_needs_a_file():
    from boosting_nerv_amd import train_nerv_all as T
    with pytest.raises(ValueError, match="--bitstream_sparse"):
        T.main("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV --crop_list 180_320 -e 1 --bitstream_sparse".split())


# ---------------------------------------------------------------------------------------------------------------------- end to end
_RECIPES = {
    "HNeRV": ("--model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
              "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 --lr 0.001"),
    "NeRV_Boost": ("--model NeRV_Boost --optim_type Adan --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 --act sin --norm none --loss Fusion10_freq "
                   "--embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 --lr 0.003"),
}


@pytest.mark.isolated
@pytest.mark.parametrize("name", ["HNeRV", "NeRV_Boost"])
def test_cli_pruned_run_writes_a_sparse_file_that_decodes_to_the_dumped_images(name, tmp_path, monkeypatch):
    """The tiny recipe with two prune events, --dump_images --bitstream t.bnrz --bitstream_sparse: `codec decode` gives the PNGs of
    visualize_model_quant byte for byte, eager and with the graph; every decoded weight tensor is zero exactly where the trained one is;
    the file's symbol bits are the bits of the report; --eval_only on the same checkpoint without the flag writes a larger .bnrq."""
    from PIL import Image
    from boosting_nerv_amd import codec, zstream
    from boosting_nerv_amd import train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    seen = []
    report = T._huffman_report

    def spy(args, *rest):
        report(args, *rest)
        seen.append((args.bits_per_param, args.full_bits_per_param))

    monkeypatch.setattr(T, "_huffman_report", spy)
    base = (f"--data_path synthetic:4x180x320 --vid tiny {_RECIPES[name]} --crop_list 180_320 --resize_list -1 --modelsize 0.05 --lower_width 6 -b 1 "
            "--eval_freq 1 -p 2 -e 2 --outf t")
    T.main((base + " --not_resume --prune_sparsity 0.4 --prune_steps 0 1 --dump_images --bitstream t.bnrz --bitstream_sparse").split())
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    path = str(tmp_path / "t.bnrz")
    budget = zstream.info(path)
    size = os.path.getsize(path)
    log = (out / "rank0.txt").read_text().splitlines()
    line = [x for x in log if x.startswith("Bitstream ")]
    assert len(line) == 1 and f"{size} bytes = {8 * size} bits" in line[0] and f"Huffman codes {budget['symbol_bits']} " in line[0]
    assert f"parse {budget['zero_parse']}" in line[0] and f"{budget['n_zero_elements']} zero elements" in line[0]
    assert len(seen) == 1 and budget["symbol_bits"] == seen[0][0] * budget["n_symbols"]
    ck = torch.load(out / "model_latest.pth", map_location="cpu")
    trained = ck["state_dict"]
    zeros = sum(int((v == 0).sum()) for k, v in trained.items() if v.dim() > 1 and "encoder" not in k)
    assert budget["n_zero_elements"] == zeros >= 0.39 * sum(v.numel() for k, v in trained.items() if v.dim() > 1 and "encoder" not in k)
    for use_graph in (False, True):
        dec = codec.Decoder(path, DEV, use_graph=use_graph)
        assert dec.kind == "sparse" and len(dec) == 4
        for i in range(4):
            png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
            assert len(png) == 1, png
            assert np.array_equal(dec.decode_u8(i), np.asarray(Image.open(png[0]))), (use_graph, i)
    n_sparse = 0
    for k, v in dec.model.state_dict().items():
        if "encoder" not in k and v.dim() > 1:
            assert torch.equal(v.cpu() == 0, trained[k] == 0), k
            assert not torch.signbit(v.cpu()[trained[k] == 0]).any(), k
            n_sparse += 1
    assert n_sparse >= 4
    frames = tmp_path / "frames"
    assert codec.main(["decode", path, "--out", str(frames)]) == 4 and codec.main(["info", path]) == budget
    for i in range(4):
        png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
        assert np.array_equal(np.asarray(Image.open(frames / f"frame_{i:04d}.png")), np.asarray(Image.open(png[0]))), i
    # the same checkpoint without the flag: the dense kind, larger, and a report that counts more bits
    T.main((base + " --eval_only --bitstream t.bnrq").split())
    dense = codec.info(str(tmp_path / "t.bnrq"))
    print(f"{name}: .bnrz {budget['bytes']} bytes ({seen[0][0]:.3f} bits per parameter, parse {budget['zero_parse']}), .bnrq {dense['bytes']} bytes ({seen[1][0]:.3f})")
    assert "zero_parse" not in dense and dense["n_symbols"] == budget["n_symbols"] and dense["bytes"] > budget["bytes"]
    assert len(seen) == 2 and dense["symbol_bits"] == seen[1][0] * dense["n_symbols"] > budget["symbol_bits"]
