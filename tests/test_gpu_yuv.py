"""Raw YUV 4:2:0 video in and out on the GPU (``-m gpu``): the two conversion kernels against the float64 restatement
(boosting_nerv_amd/yuvio.py), the loader, the decoder's raw-video packing node and the two command lines.  Fixtures are made here from
seeded random samples or the synthetic clip; nothing is committed."""
import io
import os

import numpy as np
import pytest
import torch

from boosting_nerv_amd import yuvio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOAD_TOL = 2e-6      # the up-sampling is exact in fp32; what remains is about four roundings of values below 2.1 (< 6e-7), with room for contraction choices


def _planes(gen, n, h, w, depth):
    """n frames of seeded random samples over the whole code range, the range ends included."""
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    frames = []
    for _ in range(n):
        f = [gen.integers(0, 2 ** depth, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        for p in f:
            p.reshape(-1)[0], p.reshape(-1)[-1] = 2 ** depth - 1, 0
        frames.append(tuple(f))
    return frames


def _file_bytes(frames, stride=None):
    """The frames as they lie in a file (stride: bytes from one frame's start to the next; the gap is filled with 0xff)."""
    out = []
    for f in frames:
        b = b"".join(p.tobytes() for p in f)
        out.append(b + b"\xff" * ((stride or len(b)) - len(b)))
    return np.frombuffer(b"".join(out), dtype=np.uint8)


def _reference_rgb(frames, coeffs, crop):
    return np.stack([yuvio.to_rgb_reference(*f, coeffs, crop) for f in frames])


# ---------------------------------------------------------------------------------------------------------------------- yuv420 -> rgb
# (src_h, src_w, crop): a (ch, cw) crop is the reference's centre crop; the (top, left, ch, cw) windows put top and / or left on odd source rows and columns
LOAD_SHAPES = [(2, 2, (2, 2)), (6, 10, (3, 5)), (18, 34, (18, 34)), (64, 96, (64, 96)), (6, 10, (1, 3, 3, 5)), (18, 34, (3, 1, 13, 30)), (18, 34, (2, 5, 16, 29))]


def _window(h, w, crop):
    return (*yuvio.crop_offsets(h, w, *crop), *crop) if len(crop) == 2 else crop


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("rng_name", ["limited", "full"])
def test_yuv420_to_rgb_equals_the_restatement(depth, matrix, rng_name):
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(21)
    c = yuvio.coefficients(matrix, rng_name, depth)
    for h, w, crop in LOAD_SHAPES:
        win = _window(h, w, crop)
        frames = _planes(gen, 1, h, w, depth)
        got = ops.yuv420_to_rgb(torch.from_numpy(_file_bytes(frames).copy()).to(DEV), c, 1, h, w, crop=win)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, win[2], win[3])
        want = _reference_rgb(frames, c, win)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        assert err <= LOAD_TOL, (depth, matrix, rng_name, h, w, win, err)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


@pytest.mark.parametrize("depth", [8, 10])
def test_yuv420_to_rgb_batch_with_a_frame_stride(depth):
    """B = 3 frames whose stride is larger than a frame (and breaks every alignment wider than a sample)."""
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(22)
    c = yuvio.coefficients("bt709", "limited", depth)
    h, w = 18, 34
    frames = _planes(gen, 3, h, w, depth)
    frame = yuvio.frame_samples(h, w) * c.bytes_per_sample
    stride = frame + 7 * c.bytes_per_sample
    src = torch.from_numpy(_file_bytes(frames, stride).copy()).to(DEV)
    got = ops.yuv420_to_rgb(src, c, 3, h, w, frame_stride_bytes=stride)
    assert np.abs(got.cpu().numpy().astype(np.float64) - _reference_rgb(frames, c, None)).max() <= LOAD_TOL
    win = (1, 2, 16, 31)
    got = ops.yuv420_to_rgb(src, c, 3, h, w, crop=win, frame_stride_bytes=stride)
    assert np.abs(got.cpu().numpy().astype(np.float64) - _reference_rgb(frames, c, win)).max() <= LOAD_TOL
    with pytest.raises(ValueError, match="do not fit"):
        ops.yuv420_to_rgb(src, c, 4, h, w, frame_stride_bytes=stride)


@pytest.mark.parametrize("depth", [8, 10])
def test_yuv420_to_rgb_on_operands_off_their_alignment(depth):
    """The source one sample and the output 4 bytes into their buffers: every access takes its element-by-element form; the bytes
    around the output view are not touched."""
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(23)
    c = yuvio.coefficients("bt709", "limited", depth)
    for h, w in ((64, 96), (18, 34)):
        frames = _planes(gen, 2, h, w, depth)
        raw = _file_bytes(frames)
        buf = torch.zeros(raw.size + c.bytes_per_sample, dtype=torch.uint8, device=DEV)
        buf[c.bytes_per_sample:] = torch.from_numpy(raw.copy()).to(DEV)
        src = buf[c.bytes_per_sample:]
        assert src.data_ptr() % 16 == c.bytes_per_sample
        ob = torch.full((2 * 3 * h * w + 2,), float("nan"), device=DEV)
        out = ob[1:-1].view(2, 3, h, w)
        assert out.data_ptr() % 16 == 4
        ops.yuv420_to_rgb(src, c, 2, h, w, out=out)
        assert np.abs(out.cpu().numpy().astype(np.float64) - _reference_rgb(frames, c, None)).max() <= LOAD_TOL
        assert torch.isnan(ob[0]).item() and torch.isnan(ob[-1]).item()
        aligned = ops.yuv420_to_rgb(torch.from_numpy(raw.copy()).to(DEV), c, 2, h, w)
        assert torch.equal(aligned, out)                      # the access form changes no bit


# ---------------------------------------------------------------------------------------------------------------------- rgb -> yuv420
STORE_SHAPES = [(1, 2, 2), (1, 4, 6), (1, 18, 34), (1, 64, 96), (3, 18, 34)]
TIE_WINDOW = 1e-3            # in units of s = 2^(depth - 8) codes: the fp32 error of a pre-rounding value is about 1.5e-4 s
TIE_SHARE = 0.015            # the float64 restatement alone puts 0 .. 0.7 % of seeded uniform samples inside the window at these shapes


def _check_codes(got_bytes, x, coeffs, share_bound=None):
    """got_bytes: [B, frame bytes] uint8 from the kernel; x: the fp32 input as numpy.  Codes equal wherever the float64 pre-rounding value
    is farther than TIE_WINDOW * s from a rounding tie, within 1 inside that window; the share of samples inside it stays small."""
    B, _, H, W = x.shape
    s = 2 ** (coeffs.depth - 8)
    codes, pre = yuvio.to_yuv_reference(x.astype(np.float64), coeffs, return_pre=True)
    want = np.concatenate([p.reshape(B, -1) for p in codes], axis=1).astype(np.int64)
    pre = np.concatenate([p.reshape(B, -1) for p in pre], axis=1)
    got = np.ascontiguousarray(got_bytes).view(coeffs.dtype).reshape(B, -1).astype(np.int64)
    assert got.shape == want.shape == (B, yuvio.frame_samples(H, W))
    frac = pre + 0.5 - np.floor(pre + 0.5)
    near = np.minimum(frac, 1.0 - frac) < TIE_WINDOW * s
    diff = np.abs(got - want)
    share = float(near.mean())
    print(f"  {B}x{H}x{W} {coeffs}: {int((diff > 0).sum())} of {diff.size} codes differ, {share:.4%} of the samples within {TIE_WINDOW * s:g} of a tie")
    assert (diff[~near] == 0).all(), (coeffs, x.shape, int((diff[~near] > 0).sum()), int(diff.max()))
    assert diff.max(initial=0) <= 1
    if share_bound is not None:
        assert share < share_bound, share


@pytest.mark.parametrize("depth", [8, 10])
def test_rgb_to_yuv420_equals_the_restatement(depth):
    from boosting_nerv_amd import ops
    c = yuvio.coefficients("bt709", "limited", depth)
    gen = torch.Generator().manual_seed(31 + depth)
    for B, H, W in STORE_SHAPES:
        x = torch.rand(B, 3, H, W, generator=gen)
        got = ops.rgb_to_yuv420(x.to(DEV), c)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, yuvio.frame_samples(H, W) * c.bytes_per_sample)
        _check_codes(got.cpu().numpy(), x.numpy(), c, TIE_SHARE)
    # an fp32 view 4 bytes into its buffer, and an output with a frame stride that breaks the alignment of every packed store
    x = torch.rand(2, 3, 64, 96, generator=gen)
    buf = torch.empty(x.numel() + 1, device=DEV)
    buf[1:] = x.reshape(-1).to(DEV)
    xd = buf[1:].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    got = ops.rgb_to_yuv420(xd, c)
    _check_codes(got.cpu().numpy(), x.numpy(), c, TIE_SHARE)
    assert torch.equal(got, ops.rgb_to_yuv420(x.to(DEV), c))
    frame = got.shape[1]
    stride = frame + 3 * c.bytes_per_sample
    wide = torch.full((2, stride), 0xAB, dtype=torch.uint8, device=DEV)
    ops.rgb_to_yuv420(xd, c, out=wide, frame_stride_bytes=stride)
    assert torch.equal(wide[:, :frame], got) and (wide[:, frame:] == 0xAB).all().item()


@pytest.mark.parametrize("matrix,rng_name,depth", [("bt601", "full", 8), ("bt601", "limited", 10), ("bt709", "full", 10)])
def test_rgb_to_yuv420_other_matrices_and_ranges(matrix, rng_name, depth):
    from boosting_nerv_amd import ops
    c = yuvio.coefficients(matrix, rng_name, depth)
    x = torch.rand(2, 3, 18, 34, generator=torch.Generator().manual_seed(33))
    _check_codes(ops.rgb_to_yuv420(x.to(DEV), c).cpu().numpy(), x.numpy(), c, TIE_SHARE)


@pytest.mark.parametrize("depth", [8, 10])
def test_rgb_to_yuv420_clamps_out_of_range_inputs(depth):
    from boosting_nerv_amd import ops
    c = yuvio.coefficients("bt709", "limited", depth)
    s = 2 ** (depth - 8)
    x = torch.rand(1, 3, 18, 34, generator=torch.Generator().manual_seed(34)) * 1.6 - 0.3        # about a fifth of the values on either side of [0, 1]
    _check_codes(ops.rgb_to_yuv420(x.to(DEV), c).cpu().numpy(), x.numpy(), c)
    for value, code in ((7.5, 235 * s), (-3.0, 16 * s), (float("inf"), 235 * s), (-1e30, 16 * s)):
        got = ops.rgb_to_yuv420(torch.full((1, 3, 4, 6), value, device=DEV), c).cpu().numpy().view(c.dtype).reshape(-1)
        assert (got[:24] == code).all() and (got[24:] == 128 * s).all(), (value, got)


# ---------------------------------------------------------------------------------------------------------------------- both kernels, the loader
@pytest.mark.parametrize("depth", [8, 10])
def test_flat_colours_round_trip_through_file_loader_and_store(tmp_path, depth):
    """Codes written by yuvio.write, loaded by YuvFile.to_device (5 frames in chunks of 2: both staging buffers are used twice), stored
    again: at most one code off.  The colours lie inside the RGB cube (checked with the restatement), so no clamp loses them."""
    from boosting_nerv_amd import ops
    s = 2 ** (depth - 8)
    c = yuvio.coefficients("bt709", "limited", depth)
    h, w = 8, 12
    colours = [(120, 100, 150), (200, 128, 128), (17, 128, 128), (234, 128, 128), (150, 140, 110)]
    frames = [tuple(np.full(shape, k * s, dtype=c.dtype) for k, shape in zip(col, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))) for col in colours]
    ref = _reference_rgb(frames, c, None)
    assert ref.min() > 0.0 and ref.max() < 1.0
    path = tmp_path / f"flat_{w}x{h}_{depth}bit.yuv"
    yuvio.write(path, frames, c.pix_fmt)
    clip = yuvio.YuvFile(path)
    dev = clip.to_device(DEV, chunk=2)
    assert tuple(dev.shape) == (5, 3, h, w) and np.abs(dev.cpu().numpy().astype(np.float64) - ref).max() <= LOAD_TOL
    back = ops.rgb_to_yuv420(dev, c).cpu().numpy().view(c.dtype).reshape(5, -1).astype(np.int64)
    want = np.frombuffer(path.read_bytes(), dtype=c.dtype).reshape(5, -1).astype(np.int64)
    assert np.abs(back - want).max() <= 1
    # a cropped, shortened load is the window of the same frames
    part = clip.to_device(DEV, chunk=32, crop=(5, 7), count=3)
    win = (*yuvio.crop_offsets(h, w, 5, 7), 5, 7)
    assert tuple(part.shape) == (3, 3, 5, 7) and np.abs(part.cpu().numpy().astype(np.float64) - _reference_rgb(frames[:3], c, win)).max() <= LOAD_TOL


# ---------------------------------------------------------------------------------------------------------------------- decoder
def _encoded(name):
    import test_gpu_codec as G                                # the tiny 180x320 bitstreams, built once per session
    return G._encoded(name), G.N_FRAMES, G.HW


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["NeRV_Boost", "HNeRV_Boost"])
def test_frames_yuv_are_the_store_kernel_on_the_decoded_frames(name, use_graph):
    from boosting_nerv_amd import codec, ops
    ref, n, hw = _encoded(name)
    for pack, (matrix, rng_name) in (("yuv420p", ("bt709", "limited")), ("yuv420p10le", ("bt601", "full"))):
        dec = codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=use_graph, pack=pack, matrix=matrix, range=rng_name)
        c = yuvio.coefficients(matrix, rng_name, yuvio.PIX_FMTS[pack])
        assert dec.pack == pack and len(dec) == n
        want = []
        for i in range(n):
            f32 = dec.decode_f32(i)
            assert torch.equal(f32, ref["want"][i])
            want.append(ops.rgb_to_yuv420(f32, c)[0].cpu().numpy().view(c.dtype))
        for i in (2, 0, 3, 1):
            got = dec.decode_yuv(i)
            assert got.dtype == c.dtype and got.shape == (yuvio.frame_samples(*hw),) and np.array_equal(got, want[i]), (name, pack, i)
        count = 0
        for i, got in enumerate(dec.frames_yuv()):
            assert np.array_equal(got, want[i]), (name, pack, i)
            count += 1
        assert count == n
        y, u, v = dec.split_planes(want[0])
        assert y.shape == hw and u.shape == v.shape == (hw[0] // 2, hw[1] // 2)
        with pytest.raises(RuntimeError, match="rgb8"):
            dec.decode_u8(0)


def test_rgb8_pack_is_unchanged_and_the_default():
    from boosting_nerv_amd import codec, ops
    from boosting_nerv_amd.engine import FrameDecodeGraph
    ref, n, hw = _encoded("NeRV_Boost")
    dec = codec.Decoder(io.BytesIO(ref["blob"]), DEV)
    assert dec.pack == "rgb8" and dec._loop.pack == "rgb8" and tuple(dec._loop.u8.shape) == (1, *hw, 3)
    explicit = codec.Decoder(io.BytesIO(ref["blob"]), DEV, pack="rgb8")
    for i in range(n):
        f32, u8 = dec._launch(i)
        assert torch.equal(u8, ops.frame_to_u8(f32))
        assert torch.equal(u8[0].cpu(), torch.from_numpy(dec.decode_u8(i))) and np.array_equal(dec.decode_u8(i), explicit.decode_u8(i))
    with pytest.raises(RuntimeError, match="yuv420"):
        dec.decode_yuv(0)
    with pytest.raises(ValueError, match="pack"):
        FrameDecodeGraph(dec.model, dec.norms[0:1], None, dec.norms[0:1], hw, use_graph=False, pack="yuv444p")


@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv420p10le"])
def test_cli_decode_to_a_raw_file_and_score_it(tmp_path, pix_fmt, capsys):
    """`codec decode --format yuv` writes N * 1.5 * H * W samples that YuvFile reads back as the decoder's frames; `codec psnr` of the
    stream against that very file finds no error on any plane."""
    from boosting_nerv_amd import codec
    ref, n, hw = _encoded("HNeRV_Boost")
    depth = yuvio.PIX_FMTS[pix_fmt]
    stream = tmp_path / "tiny.bnrv"
    stream.write_bytes(ref["blob"])
    out = tmp_path / f"dec_{hw[1]}x{hw[0]}_{depth}bit.yuv"
    assert codec.main(["decode", str(stream), "--out", str(out), "--format", "yuv", "--pix_fmt", pix_fmt]) == n
    bps = 1 if depth == 8 else 2
    assert os.path.getsize(out) == n * hw[0] * hw[1] * 3 // 2 * bps
    clip = yuvio.YuvFile(out)
    assert (len(clip), clip.height, clip.width, clip.pix_fmt) == (n, hw[0], hw[1], pix_fmt)
    dec = codec.Decoder(str(stream), DEV, pack=pix_fmt)
    for i in range(n):
        for got, want in zip(clip.planes(i), dec.split_planes(dec.decode_yuv(i))):
            assert np.array_equal(got, want)
    result = codec.main(["psnr", str(stream), "--ref", str(out)])
    assert result["sse_y"] == result["sse_u"] == result["sse_v"] == 0 and result["frames"] == n and result["pix_fmt"] == pix_fmt
    assert result["psnr_y"] == result["psnr_yuv"] == float("inf")
    assert "PSNR-YUV" in capsys.readouterr().out
    # another matrix is another file: the score is finite
    other = codec.main(["psnr", str(stream), "--ref", str(out), "--matrix", "bt601"])
    assert other["sse_y"] + other["sse_u"] + other["sse_v"] > 0 and np.isfinite(other["psnr_yuv"])


# ---------------------------------------------------------------------------------------------------------------------- train CLI
NERV_LINE = ("--vid tiny --model NeRV_Boost --sft_block res_sft --ch_t 32 --conv_type convnext pshuffel_3x3 --act sin --norm none --crop_list 180_320 "
             "--resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --fc_hw 9_16 --dec_strds 5 2 2 --ks 0_3_3 --reduce 2 --dec_blks 1 1 2 "
             "--modelsize 0.05 --lower_width 6 -b 1 --lr 0.003 -p 1 --optim_type Adan")
HNERV_LINE = ("--vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin --norm none "
              "--crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 "
              "--reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 --lr 0.002 --lr_type cosine_0_1_0.1 -p 1")


@pytest.mark.isolated
@pytest.mark.parametrize("line,depth", [(NERV_LINE, 8), (HNERV_LINE, 8), (NERV_LINE, 10)], ids=["nerv_boost_8bit", "hnerv_boost_8bit", "nerv_boost_10bit"])
def test_train_cli_reads_a_raw_clip(tmp_path, monkeypatch, line, depth):
    """train_nerv_all.py --data_path clip_320x180_<depth>bit.yuv -e 1 on four frames of the synthetic clip: the captured step, a finite
    PSNR in the log, and a resident clip that is the restatement of the file."""
    from boosting_nerv_amd import synth, train_nerv_all as T
    monkeypatch.chdir(tmp_path)
    c = yuvio.coefficients("bt709", "limited", depth)
    video = synth.SyntheticVideo(4, 180, 320)
    frames = [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)]
    path = tmp_path / f"clip_320x180_{depth}bit.yuv"
    yuvio.write(path, frames, c.pix_fmt)
    seen = {}
    orig_step, orig_eval = T.TrainStep, T.evaluate

    class Spy(orig_step):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["step"] = self

    def spy_eval(model, loader, rank, args, *a, **k):
        seen["clip"] = args._frames_dev.clone()
        return orig_eval(model, loader, rank, args, *a, **k)
    monkeypatch.setattr(T, "TrainStep", Spy)
    monkeypatch.setattr(T, "evaluate", spy_eval)
    T.main((line + f" --data_path {path} --outf ty -e 1 --not_resume").split())
    assert seen["step"].graph_a is not None
    log = (tmp_path / "output" / "ty" / "tiny" / "Size0.05" / "rank0.txt").read_text()
    assert "Train step: captured" in log and "Epoch[1/1]" in log and "Eval at epoch 1" in log
    psnrs = [float(l.split("pred_PSNR: ")[1]) for l in log.splitlines() if "pred_PSNR" in l]
    assert len(psnrs) == 4 and all(np.isfinite(p) and p > 0 for p in psnrs), psnrs
    clip = seen["clip"]
    assert clip.dtype == torch.float32 and tuple(clip.shape) == (4, 3, 180, 320)
    assert np.abs(clip.cpu().numpy().astype(np.float64) - _reference_rgb(frames, c, None)).max() <= LOAD_TOL
