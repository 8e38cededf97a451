"""GPU tests (``-m gpu``) of --resize_list: the resize kernels against the host definition, the loader's device paths
against its host path, a resized run through both train scripts and their files, and `Decoder.score` of such a file against its master.
Every comparison is an equality: the kernels accumulate in the order of resize.resize_reference, product and sum rounded on their own."""
import glob
import os

import numpy as np
import pytest
import torch

from resize_cases import GEOMETRIES, IDS as _IDS, png_dir as _png_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HNERV = ("--vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 "
         "--dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 --modelsize 0.05 --lower_width 6 -b 1 --lr 0.001 -p 2 -e 1 --not_resume")
BOOST_CEM = ("--vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin --norm none "
             "--loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 "
             "--modelsize 0.05 --lower_width 6 -b 1 -e 1 --eval_freq 1 --lr 0.002 --lr_type cosine_0_1_0.1 --not_resume --embed_entropy --quant "
             "--quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale --quantizer_e scalebeta "
             "--lambda_rate 0.5 --target_bit 2 -p 1")


# ---------------------------------------------------------------------------------------------------------------------- the kernels
def _view(flat, shape, offset):
    """A contiguous view of a device buffer, starting one float past its 16-byte aligned base when `offset`."""
    n = int(np.prod(shape))
    return flat[offset:offset + n].view(*shape)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("B,C", [(1, 3), (3, 1)])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=_IDS)
def test_resize_bicubic_equals_the_definition(geom, B, C, offset):
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.resize import resize_reference
    H, W, h, w = geom
    host = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(100 * H + W + B))
    x_buf = torch.zeros(B * C * H * W + 8, device=DEV)
    x = _view(x_buf, (B, C, H, W), offset)
    x.copy_(host)
    assert x.data_ptr() % 16 == 4 * offset and x.is_contiguous()
    for clamp in (True, False):
        out_buf = torch.full((B * C * h * w + 8,), -7.0, device=DEV)
        scratch_buf = torch.full((B * C * H * w + 8,), -7.0, device=DEV)
        out, scratch = _view(out_buf, (B, C, h, w), offset), scratch_buf[offset:offset + B * C * H * w]
        got = ops.resize_bicubic(x, (h, w), clamp=clamp, out=out, scratch=scratch)
        assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 4 * offset
        want = resize_reference(host, (h, w), clamp=clamp)
        assert torch.equal(got.cpu(), want), (geom, B, C, offset, clamp)
        # nothing outside the two tensors was written
        for buf, n in ((out_buf, B * C * h * w), (scratch_buf, B * C * H * w)):
            assert (buf[:offset] == -7.0).all() and (buf[offset + n:] == -7.0).all()
        assert torch.equal(ops.resize_bicubic(x, (h, w), clamp=clamp).cpu(), want)          # buffers of its own
    if (H, W) == (h, w):
        assert torch.equal(ops.resize_bicubic(x, (h, w)), x) and torch.equal(ops.resize_bicubic(x, (h, w), clamp=False), x)
    assert torch.equal(x.cpu(), host)                                                      # the input is left alone


def test_resize_bicubic_several_strips_and_row_groups():
    """More than one strip of 64 output columns, a last strip that is not full, rows that do not fill the last block, both staging forms."""
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.resize import resize_reference
    for (H, W, h, w) in ((37, 300, 21, 150), (35, 301, 50, 131), (33, 1040, 5, 66)):
        host = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H + W))
        assert torch.equal(ops.resize_bicubic(host.to(DEV), (h, w)).cpu(), resize_reference(host, (h, w))), (H, W, h, w)


def test_resize_bicubic_refusals():
    from boosting_nerv_amd import ops
    x = torch.rand(1, 3, 12, 20, device=DEV)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.resize_bicubic(x.transpose(2, 3), (6, 10))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.resize_bicubic(x.double(), (6, 10))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.resize_bicubic(x[:0], (6, 10))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.resize_bicubic(x[0], (6, 10))
    with pytest.raises(ValueError, match="overlap"):
        ops.resize_bicubic(x, (12, 20), out=x)
    buf = torch.zeros(2 * 3 * 12 * 20, device=DEV)
    with pytest.raises(ValueError, match="overlap"):
        ops.resize_bicubic(buf[:720].view(1, 3, 12, 20), (12, 20), out=buf[716:1436].view(1, 3, 12, 20))
    with pytest.raises(ValueError, match="out must be"):
        ops.resize_bicubic(x, (6, 10), out=torch.empty(1, 3, 6, 11, device=DEV))
    with pytest.raises(ValueError, match="scratch"):
        ops.resize_bicubic(x, (6, 10), scratch=torch.empty(3 * 12 * 10 - 1, device=DEV))
    with pytest.raises(ValueError, match="size"):
        ops.resize_bicubic(x, (0, 10))
    out = torch.full((1, 1, 1, 4), -7.0, device=DEV)
    with pytest.raises(ValueError, match="taps"):                       # over the tap limit on either axis: refused before any launch
        ops.resize_bicubic(torch.rand(1, 1, 130, 4, device=DEV), (1, 4), out=out)
    with pytest.raises(ValueError, match="taps"):
        ops.resize_bicubic(torch.rand(1, 1, 4, 130, device=DEV), (4, 1))
    assert (out == -7.0).all()
    with pytest.raises(Exception, match="ROCm GPU"):
        ops.resize_bicubic(torch.rand(1, 3, 12, 20), (6, 10))


# ---------------------------------------------------------------------------------------------------------------------- the loader
def _args(data_path, **over):
    from types import SimpleNamespace
    return SimpleNamespace(data_path=data_path, crop_list="270_480", resize_list="180_320", **over)


@pytest.mark.parametrize("source", ["png", "synthetic"])
def test_to_device_equals_the_host_frames(tmp_path, source):
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    data_path = _png_dir(tmp_path / "frames", 5, 274, 486) if source == "png" else "synthetic:5x270x480"
    ds = VideoDataSet(_args(data_path))
    want = torch.stack([ds[i]["img"] for i in range(len(ds))])
    assert want.shape == (5, 3, 180, 320)
    clip = ds.to_device(DEV)
    assert clip.is_cuda and clip.dtype == torch.float32 and torch.equal(clip.cpu(), want)
    assert torch.equal(ds.to_device(DEV, chunk=3), clip)                 # two chunks, the second short
    from types import SimpleNamespace
    plain = VideoDataSet(SimpleNamespace(data_path=data_path, crop_list="270_480", resize_list="-1"))
    assert plain.to_device(DEV).shape == (5, 3, 270, 480)               # -1: the clip at the crop size, as before


def test_yuv_to_device_resizes_each_chunk(tmp_path):
    from boosting_nerv_amd import ops, yuvio
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    rng = np.random.default_rng(3)
    path = str(tmp_path / "clip_484x272_8bit.yuv")
    yuvio.write(path, [(rng.integers(16, 236, size=(272, 484), dtype=np.uint8), rng.integers(16, 241, size=(136, 242), dtype=np.uint8),
                        rng.integers(16, 241, size=(136, 242), dtype=np.uint8)) for _ in range(5)])
    clip = yuvio.YuvFile(path)
    full = clip.to_device(DEV, crop=(270, 480))
    want = ops.resize_bicubic(full, (180, 320))
    got = clip.to_device(DEV, crop=(270, 480), resize=(180, 320))
    assert got.shape == (5, 3, 180, 320) and torch.equal(got, want)
    assert torch.equal(clip.to_device(DEV, chunk=3, crop=(270, 480), resize=(180, 320)), want)
    assert torch.equal(VideoDataSet(_args(path)).to_device(DEV), want)
    assert torch.equal(VideoDataSet(_args(path)).to_device(DEV, chunk=3), want)


# ---------------------------------------------------------------------------------------------------------------------- a resized run
_runs = {}


def _hnerv_run(tmp_path_factory):
    """One epoch of the tiny HNeRV recipe on a 270x480 clip resized to 180x320, with --dump_images --bitstream: run once, shared."""
    if "hnerv" not in _runs:
        from boosting_nerv_amd import train_nerv_all as T
        root = tmp_path_factory.mktemp("resized")
        path = str(root / "t.bnrq")
        seen = {}
        orig = T.evaluate

        def spy(model, loader, rank, args, *a, **k):
            out = orig(model, loader, rank, args, *a, **k)
            seen["hw"], seen["clip"] = out[1], args._frames_dev.clone()
            return out
        cwd = os.getcwd()
        os.chdir(root)
        T.evaluate = spy
        try:
            T.main(f"--outf t --data_path synthetic:4x270x480 --crop_list 270_480 --resize_list 180_320 {HNERV} --dump_images --bitstream {path}".split())
        finally:
            T.evaluate = orig
            os.chdir(cwd)
        _runs["hnerv"] = dict(root=root, path=path, out=root / "output" / "t" / "tiny" / "Size0.05", **seen)
    return _runs["hnerv"]


def test_resized_run_logs_trains_and_decodes_at_the_resized_size(tmp_path_factory):
    from PIL import Image
    from boosting_nerv_amd import codec, qstream
    run = _hnerv_run(tmp_path_factory)
    log = (run["out"] / "rank0.txt").read_text().splitlines()
    line = [x for x in log if x.startswith("Resize:")]
    assert line == ["Resize: 270x480 -> 180x320 (antialiased bicubic), 6 x 6 taps"], line      # 1.5x: c - 2.5 and c + 3.5 share their fraction: always 4 * 1.5 = 6
    assert tuple(run["hw"]) == (180, 320) and run["clip"].shape == (4, 3, 180, 320)
    s = qstream.read(run["path"]).settings
    assert s["crop_list"] == "180_320" and s["source_crop"] == "270_480" and s["final_size"] == 180 * 320
    out_dir = run["root"] / "frames"
    assert codec.main(["decode", run["path"], "--out", str(out_dir)]) == 4
    for i in range(4):
        png = glob.glob(str(run["out"] / "visualize_model_quant" / f"pred_{i:04d}_*.png"))
        assert len(png) == 1, png
        img = Image.open(png[0])
        assert img.size == (320, 180)
        assert (out_dir / f"frame_{i:04d}.png").read_bytes() == open(png[0], "rb").read(), i
    info = codec.main(["info", run["path"]])
    assert info["source_crop"] == "270_480" and info["total"] == 8 * os.path.getsize(run["path"])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_score_of_a_resized_file_against_its_master(tmp_path_factory, tmp_path, use_graph):
    from types import SimpleNamespace
    from boosting_nerv_amd import codec, ops, synth, yuvio
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    run = _hnerv_run(tmp_path_factory)
    master = str(tmp_path / "master_480x270_8bit.yuv")
    coeffs = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(4, 270, 480)
    yuvio.write(master, [yuvio.to_yuv_reference(video.frame(i).numpy(), coeffs) for i in range(4)])
    ref = yuvio.YuvFile(master)
    dec = codec.Decoder(run["path"], DEV, use_graph=use_graph, pack="yuv420p")
    got = dec.score(ref)
    for key in ("sse", "psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "msssim_y"):
        assert got[key] is None, key
    clip = VideoDataSet(SimpleNamespace(data_path=master, crop_list="270_480", resize_list="180_320")).to_device(DEV)
    want = torch.cat([ops.psnr(dec.decode_f32(i), clip[i:i + 1]) for i in range(4)]).cpu().numpy()
    assert got["psnr_rgb"].dtype == np.float32 and np.array_equal(got["psnr_rgb"], want)
    want_ms = torch.cat([ops.msssim(dec.decode_f32(i), clip[i:i + 1]) for i in range(4)]).cpu().numpy()
    assert np.array_equal(got["msssim_rgb"], want_ms)
    assert got["mean"]["psnr_y"] is None and abs(got["mean"]["psnr_rgb"] - float(want.astype(np.float64).mean())) < 1e-4
    over = dec.score(ref, msssim=False, resize_from=(270, 480))         # the explicit override, the same numbers
    assert np.array_equal(over["psnr_rgb"], want) and over["msssim_rgb"] is None
    if use_graph:
        result = codec.main(["score", run["path"], "--ref", master])
        assert result["psnr_rgb"] == got["mean"]["psnr_rgb"] and "psnr_y" not in result and result["sse_y"] is None and result["source_crop"] == "270_480"
        with pytest.raises(ValueError, match="codec score"):
            codec.main(["psnr", run["path"], "--ref", master])


def test_compression_run_under_the_flag_decodes_to_what_it_scored(tmp_path, monkeypatch):
    from boosting_nerv_amd import bitstream, codec, ops
    from boosting_nerv_amd import train_nerv_compression as C
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / "t.bnrv")
    scored, state = [], {"in": False}
    orig_eval, orig_psnr = C.evaluate, ops.psnr

    def spy_eval(*a, **k):
        scored.clear()
        state["in"] = True
        try:
            return orig_eval(*a, **k)
        finally:
            state["in"] = False

    def spy_psnr(out, gt):
        if state["in"]:
            scored.append(out.detach().clone())
        return orig_psnr(out, gt)
    monkeypatch.setattr(C, "evaluate", spy_eval)
    monkeypatch.setattr(ops, "psnr", spy_psnr)
    C.main(f"--outf t --data_path synthetic:4x270x480 --crop_list 270_480 --resize_list 180_320 {BOOST_CEM} --bitstream {path}".split())
    monkeypatch.setattr(ops, "psnr", orig_psnr)
    log = (tmp_path / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text().splitlines()
    assert [x for x in log if x.startswith("Resize:")] == ["Resize: 270x480 -> 180x320 (antialiased bicubic), 6 x 6 taps"]
    s = bitstream.read(path).settings
    assert s["crop_list"] == "180_320" and s["source_crop"] == "270_480"
    assert bitstream.info(path)["total"] == 8 * os.path.getsize(path)
    dec = codec.Decoder(path, DEV)
    assert len(dec) == 4 == len(scored) and dec.frame_hw == (180, 320)
    for i in range(4):
        f32 = dec.decode_f32(i)
        assert f32.shape == (1, 3, 180, 320) and torch.equal(f32, scored[i]), i


def test_runs_without_the_flag_write_the_same_bytes(tmp_path, monkeypatch):
    from boosting_nerv_amd import qstream
    from boosting_nerv_amd import train_nerv_all as T
    blobs = []
    for name, flag in (("absent", ""), ("minus1", "--resize_list -1")):
        root = tmp_path / name
        root.mkdir()
        monkeypatch.chdir(root)
        path = str(root / "t.bnrq")
        T.main(f"--outf t --data_path synthetic:4x180x320 --crop_list 180_320 {flag} {HNERV} --bitstream {path}".split())
        log = (root / "output" / "t" / "tiny" / "Size0.05" / "rank0.txt").read_text()
        assert "Resize:" not in log
        assert "source_crop" not in qstream.read(path).settings
        blobs.append(open(path, "rb").read())
    assert blobs[0] == blobs[1]
