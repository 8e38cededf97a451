"""The post-hoc quantised model's file on the GPU (``-m gpu``): the decode kernel against the host coder and the
numpy restatement, bit for bit; quant_model -> encode_posthoc -> Decoder equals the frames evaluate() scores for the twin; and one
train_nerv_all --bitstream run whose file decodes to the dumped PNGs.  Every stream here is valid: damaged input is the host coder's
business (test_qstream_cpu.py)."""
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import configs
import hnerv_ref
import qstream_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_shared = {}


def _run(records, offset=False, lengths=None):
    """Code the host records, decode them with ONE ops.huff_dequant launch, return the outputs (and their guard elements).  offset: every
    output is a view one element into its buffer -- 4 bytes off a 16-byte boundary."""
    from boosting_nerv_amd import ops
    words, lengths, split = Q.stream(records, lengths)
    items, bufs = [], []
    for (q, lo, step, outer, red, inner, flag), rb in zip(records, split):
        buf = torch.full((q.size + 2 if offset else q.size,), float("nan"), device=DEV)
        out = buf[1:1 + q.size] if offset else buf
        assert out.data_ptr() % 16 == (4 if offset else 0)
        items.append((out, torch.from_numpy(lo).to(DEV), torch.from_numpy(step).to(DEV), red, inner, rb))
        bufs.append(buf)
    ops.huff_dequant(words, lengths, items)
    return [it[0] for it in items], bufs, lengths


def _check(records, outs):
    for k, (rec, out) in enumerate(zip(records, outs)):
        want = torch.from_numpy(Q.restate(*rec[:6]))
        assert torch.equal(out.cpu(), want), (k, rec[3:], int((out.cpu() != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------- kernel against host
def test_kernel_equals_rebuilt_on_the_five_quant_tensor_records():
    five = Q.five_records()
    records = [r for r, _ in five]
    outs, _, _ = _run(records)
    _check(records, outs)
    for k, ((_, rebuilt), out) in enumerate(zip(five, outs)):
        assert torch.equal(out.cpu(), torch.from_numpy(rebuilt)), k


def test_kernel_hand_built_grids_both_dtypes():
    rng = np.random.default_rng(21)
    records = [Q.hand_record(g, flag, rng) for flag in (Q.F32, Q.F16) for g in ((3, 5, 7), (2, 300, 3), (1, 9, 40), (7, 1, 1), 513)]
    outs, _, _ = _run(records)
    _check(records, outs)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 64 * 256 - 1, 64 * 256 + 1])
def test_kernel_element_counts(n):
    rng = np.random.default_rng(n)
    gauss = np.rint(rng.normal(120, 25, size=n)).clip(0, 255).astype(np.uint8)
    records = [Q.hand_record(n, Q.F32, rng, gauss)]
    outs, _, _ = _run(records)
    _check(records, outs)


def test_kernel_thirty_small_items_share_a_block_and_an_item_straddles_blocks():
    rng = np.random.default_rng(22)
    records = [Q.hand_record(3, Q.F16 if k % 2 else Q.F32, rng) for k in range(30)]
    records += [Q.hand_record((4, 640, 1), Q.F16, rng), Q.hand_record((1, 100, 256), Q.F16, rng)]      # runs 30..39, then 40..139: over the 64-run block edge
    outs, _, _ = _run(records)
    _check(records, outs)


def test_kernel_outputs_four_bytes_off_a_sixteen_byte_boundary():
    rng = np.random.default_rng(23)
    records = [Q.hand_record(n, Q.F32, rng) for n in (5, 256, 1000)] + [Q.hand_record((3, 50, 4), Q.F16, rng)]
    outs, bufs, _ = _run(records, offset=True)
    _check(records, outs)
    for buf in bufs:                                        # the elements around every view were not touched
        assert torch.isnan(buf[0]).item() and torch.isnan(buf[-1]).item()


def test_kernel_depth_16_alphabet_and_one_symbol_alphabet():
    from boosting_nerv_amd import _lib as L
    rng = np.random.default_rng(24)
    deep = [Q.hand_record(65535, Q.F32, rng, Q.depth16_symbols())]
    outs, _, lengths = _run(deep)
    assert lengths.max() == 16 > L.HUFF_LUT_BITS            # codes past the first-level table: the canonical search
    _check(deep, outs)
    one = [Q.hand_record(300, Q.F16, rng, np.full(300, 7, dtype=np.uint8))]
    outs, _, lengths = _run(one)
    assert lengths[7] == 1 and lengths[256] == 1 and lengths.sum() == 2
    _check(one, outs)


def test_kernel_reads_from_memory_when_a_block_of_runs_outgrows_its_lds_span():
    """A valid but wasteful code -- lengths 1, 2, ..., 19, 20, 20 -- and data made of its 17- to 20-bit symbols only: 64 full runs hold more than
    the 8192 words a block stages in LDS, so the first block takes the path that fetches its words from memory; the short last block stages."""
    lengths = np.zeros(257, dtype=np.uint8)
    lengths[:19] = np.arange(1, 20)
    lengths[19] = lengths[256] = 20
    rng = np.random.default_rng(26)
    n = 70 * 256 + 9
    rec = Q.hand_record((1, n, 1), Q.F16, rng, rng.integers(16, 20, size=n).astype(np.uint8))
    outs, _, _ = _run([rec], lengths=lengths)
    words, _, split = Q.stream([rec], lengths)
    assert int(split[0][:64].sum(dtype=np.int64)) > 32 * 8192 and int(split[0][64:].sum(dtype=np.int64)) < 32 * 8000
    _check([rec], outs)


def test_huff_dequant_refuses_bad_items_before_any_launch():
    from boosting_nerv_amd import ops
    rng = np.random.default_rng(25)
    rec = Q.hand_record(300, Q.F32, rng)
    words, lengths, split = Q.stream([rec])
    out, lo, step = torch.zeros(300, device=DEV), torch.from_numpy(rec[1]).to(DEV), torch.from_numpy(rec[2]).to(DEV)
    with pytest.raises(ValueError, match="run lengths for"):
        ops.huff_dequant(words, lengths, [(out, lo, step, 300, 1, split[0][:1])])
    with pytest.raises(ValueError, match="slices"):
        ops.huff_dequant(words, lengths, [(out, lo, step, 7, 1, split[0])])
    with pytest.raises(ValueError, match="fp32 tensor"):
        ops.huff_dequant(words, lengths, [(out.double(), lo, step, 300, 1, split[0])])
    with pytest.raises(ValueError, match="add up"):
        ops.huff_dequant(words[:-1], lengths, [(out, lo, step, 300, 1, split[0])])
    with pytest.raises(ValueError, match="runs of 256"):
        ops.huff_dequant(words, lengths, [(out, lo, step, 300, 1, split[0])], run=128)


# ---------------------------------------------------------------------------------------------------------------------- end to end
N_FRAMES, HW = 4, (180, 320)


def _hnerv_base():
    a = hnerv_ref.tiny_args()
    a.model = "HNeRV"
    return a


_CONFIGS = {"NeRV_Boost": configs.tiny_nerv, "ENeRV_Boost": configs.tiny_enerv, "HNeRV_Boost": configs.tiny_hnerv, "HNeRV": _hnerv_base}


def _encoded(name):
    """One tiny model per architecture with seeded, perturbed weights; evaluate()'s steps for the quantised twin at -b 1 -- quant_model, the
    fp32 model's embeddings quantised as one [N, C, h, w] tensor, the twin's forward of every frame -- computed once; then encode_posthoc."""
    if name in _shared:
        return _shared[name]
    from boosting_nerv_amd import codec
    from boosting_nerv_amd import train_nerv_all as T
    from boosting_nerv_amd.hnerv_utils import quant_tensor
    from boosting_nerv_amd.synth import SyntheticVideo
    args = _CONFIGS[name]()
    args.__dict__.update(quant_model_bit=8, quant_embed_bit=6, crop_list="180_320", final_size=HW[0] * HW[1], full_data_length=N_FRAMES, batchSize=1)
    torch.manual_seed(3)
    model = T.build_model(args).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(1.0 + 0.5 * torch.rand_like(p))
    vid = SyntheticVideo(N_FRAMES, *HW)
    frames = torch.stack([vid.frame(i) for i in range(N_FRAMES)]).to(DEV)
    is_hnerv = "HNeRV" in name
    takes_image = "pe" not in args.embed or "HNeRV_Boost" in name
    norms = [torch.tensor([float(i + 1) / N_FRAMES], dtype=torch.float64, device=DEV) for i in range(N_FRAMES)]
    with torch.no_grad():
        (plain, twin), records = T.quant_model(model, args)
        plain.eval(), twin.eval()
        quant_embed, deq = None, [None] * N_FRAMES
        if is_hnerv:
            embeds = [plain(frames[i:i + 1], None, norm_idx=norms[i])[1][0] for i in range(N_FRAMES)]
            quant_embed, d = quant_tensor(torch.cat(embeds, 0), args.quant_embed_bit)
            deq = d.split(1, dim=0)
        want = [twin(frames[i:i + 1] if takes_image else norms[i], deq[i], norm_idx=norms[i])[0].clone() for i in range(N_FRAMES)]
    buf = io.BytesIO()
    budget = codec.encode_posthoc(model, args, records, quant_embed, buf)
    recs = ([quant_embed] if is_hnerv else []) + list(records.values())
    flat = torch.cat([r["quant"].flatten().cpu() for r in recs]).to(torch.int64)
    hist = torch.bincount(flat, minlength=1)
    _shared[name] = dict(blob=buf.getvalue(), budget=budget, want=want, bits=T._huffman_total_bits(hist[hist > 0].tolist()), numel=flat.numel(),
                         n_records=len(recs))
    return _shared[name]


def _pack_ref(x):
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["NeRV_Boost", "ENeRV_Boost", "HNeRV_Boost", "HNeRV"])
def test_decoded_frames_equal_the_twin_evaluate_scores(name, use_graph):
    from boosting_nerv_amd import codec
    ref = _encoded(name)
    dec = codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=use_graph)
    assert dec.kind == "posthoc" and len(dec) == N_FRAMES and dec.frame_hw == HW
    for i in (2, 0, 1, 3):
        got = dec.decode_f32(i)
        assert torch.equal(got, ref["want"][i]), (name, i, (got - ref["want"][i]).abs().max().item())
        assert np.array_equal(dec.decode_u8(i), _pack_ref(ref["want"][i])[0].cpu().numpy()), (name, i)
    for i, u8 in enumerate(dec):
        assert np.array_equal(u8, _pack_ref(ref["want"][i])[0].cpu().numpy()), (name, i)
    assert i == N_FRAMES - 1


@pytest.mark.parametrize("name", ["NeRV_Boost", "ENeRV_Boost", "HNeRV_Boost", "HNeRV"])
def test_symbol_bits_of_the_file_are_the_bits_the_huffman_report_counts(name):
    from boosting_nerv_amd import qstream
    ref = _encoded(name)
    budget = qstream.info(ref["blob"])
    print(f"{name}: {budget}, _huffman_total_bits {ref['bits']} over {ref['numel']} symbols")
    assert budget == ref["budget"] and budget["symbol_bits"] == ref["bits"] and budget["n_symbols"] == ref["numel"]
    assert budget["total"] == 8 * len(ref["blob"]) and budget["n_records"] == ref["n_records"]
    s = qstream.read(ref["blob"]).settings
    assert s["model"] == name and s["full_data_length"] == N_FRAMES and s["crop_list"] == "180_320" and s["final_size"] == 180 * 320
    assert ("embed_shape" in s) == ("HNeRV" in name)


def test_decoder_packs_yuv_from_a_posthoc_file():
    """The packing modes sit behind the same forward: yuv420p of a decoded frame is the conversion kernel on decode_f32."""
    from boosting_nerv_amd import codec, ops, yuvio
    ref = _encoded("NeRV_Boost")
    dec = codec.Decoder(ref["blob"], DEV, use_graph=False, pack="yuv420p")
    want = ops.rgb_to_yuv420(ref["want"][1], yuvio.coefficients("bt709", "limited", 8))[0].cpu().numpy()
    assert np.array_equal(dec.decode_yuv(1), want)


# ---------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_train_with_bitstream_decodes_to_the_dumped_images(tmp_path):
    """train_nerv_all.py --dump_images --bitstream in a child process: the decoded bytes of every frame ARE the PNG the final evaluation
    wrote for the quantised twin, and the log carries the budget of the file."""
    from PIL import Image
    from boosting_nerv_amd import codec, qstream
    path = str(tmp_path / "f.bnrq")
    flags = ("--outf t --data_path synthetic:4x180x320 --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none "
             "--crop_list 180_320 --resize_list -1 --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 "
             f"--modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 --eval_freq 1 -p 2 -e 1 --not_resume --dump_images --bitstream {path}")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_nerv_all.py")] + flags.split(), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = tmp_path / "output" / "t" / "tiny" / "Size0.05"
    budget = qstream.info(path)
    size = os.path.getsize(path)
    log = (out / "rank0.txt").read_text().splitlines()
    line = [x for x in log if x.startswith("Bitstream ")]
    assert len(line) == 1 and f"{size} bytes = {8 * size} bits" in line[0] and f"Huffman codes {budget['symbol_bits']} " in line[0]
    assert any("bits per parameter" in x for x in log[:log.index(line[0])])           # under the Huffman line
    dec = codec.Decoder(path, DEV)
    assert len(dec) == 4
    for i in range(4):
        png = glob.glob(str(out / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
        assert len(png) == 1, png
        assert np.array_equal(dec.decode_u8(i), np.asarray(Image.open(png[0]))), i
    assert codec.main(["info", path]) == budget
