"""Scoring a bitstream against its raw source on the GPU (``-m gpu``): the two kernels of csrc/yuv.hip behind
ops.yuv420_sse / ops.yuv_luma_f32 against yuvio.psnr_planes (exact integers) and the numpy division (exact bits), MS-SSIM-Y against the
independent float64 form, codec.Decoder.score against the host path of `codec psnr`, and the `codec score` command on files the train
scripts write from a raw clip.  Fixtures are made here from seeded random samples or the synthetic clip; nothing is committed."""
import csv
import io
import json

import numpy as np
import pytest
import torch

from boosting_nerv_amd import yuvio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (H, W) of the packed frames, (src_h, src_w) of the source (None: the frames' own size), (top, left) of the window (even).  16-byte strips
# hold 16 samples at 8 bits and 8 at 10: the rows cover strip tails, rows shorter than a strip and a `left` that is 2 mod 16.
SSE_SHAPES = [((2, 2), None, (0, 0)), ((6, 10), None, (0, 0)), ((18, 34), None, (0, 0)), ((64, 96), None, (0, 0)),
              ((16, 28), (18, 34), (2, 2)), ((12, 30), (18, 34), (4, 0)), ((16, 16), (64, 96), (24, 40))]


def _planes(gen, n, h, w, depth):
    """n frames of seeded random samples over the whole code range, the range ends included (test_gpu_yuv._planes)."""
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


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).copy()).to(DEV)


def _window_of(frame, top, left, h, w):
    y, u, v = frame
    return (y[top:top + h, left:left + w], u[top // 2:(top + h) // 2, left // 2:(left + w) // 2], v[top // 2:(top + h) // 2, left // 2:(left + w) // 2])


def _want_sse(a_frames, b_frames, top, left, h, w, depth):
    rows = []
    for fa, fb in zip(a_frames, b_frames):
        one = yuvio.psnr_planes(fa, _window_of(fb, top, left, h, w), depth)
        rows.append([one["sse_y"], one["sse_u"], one["sse_v"]])
    return rows


def _bps(depth):
    return 1 if depth == 8 else 2


# ---------------------------------------------------------------------------------------------------------------------- yuv420_sse
@pytest.mark.parametrize("depth", [8, 10])
def test_yuv420_sse_equals_psnr_planes_over_window_shapes(depth):
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(51 + depth)
    for (h, w), src, (top, left) in SSE_SHAPES:
        sh, sw = src or (h, w)
        a, b = _planes(gen, 1, h, w, depth), _planes(gen, 1, sh, sw, depth)
        got = ops.yuv420_sse(_dev(_file_bytes(a)), _dev(_file_bytes(b)), 1, h, w, _bps(depth), src_hw=src, window=(top, left))
        assert got.dtype == torch.int64 and tuple(got.shape) == (1, 3) and got.device.type == "cuda"
        want = _want_sse(a, b, top, left, h, w, depth)
        assert got.cpu().tolist() == want, (depth, h, w, src, top, left)
        assert want[0][0] > 0
    # a frame against itself, and `out` given (and not zero before the call: the call zeroes it)
    a = _planes(gen, 1, 18, 34, depth)
    out = torch.full((1, 3), 77, dtype=torch.int64, device=DEV)
    raw = _dev(_file_bytes(a))
    assert ops.yuv420_sse(raw, raw, 1, 18, 34, _bps(depth), out=out) is out and out.cpu().tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("depth", [8, 10])
def test_yuv420_sse_batch_with_padded_strides_and_sliced_operands(depth):
    """B = 3, both frame strides 6 bytes longer than a frame (later frames start 2-byte aligned only), both operands one sample off their
    allocation (8 bits: one byte); the 0xff padding between the frames is not counted."""
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(61 + depth)
    bps = _bps(depth)
    for (h, w), (sh, sw), (top, left) in (((16, 28), (18, 34), (2, 2)), ((18, 34), (18, 34), (0, 0)), ((64, 96), (64, 96), (0, 0))):
        a, b = _planes(gen, 3, h, w, depth), _planes(gen, 3, sh, sw, depth)
        sa, sb = yuvio.frame_samples(h, w) * bps + 6, yuvio.frame_samples(sh, sw) * bps + 6
        ops_in = []
        for raw in (_file_bytes(a, sa), _file_bytes(b, sb)):
            buf = torch.full((raw.size + bps,), 0xff, dtype=torch.uint8, device=DEV)
            buf[bps:] = _dev(raw)
            view = buf[bps:]
            assert view.is_contiguous() and view.data_ptr() % 16 == bps
            ops_in.append(view)
        got = ops.yuv420_sse(ops_in[0], ops_in[1], 3, h, w, bps, src_hw=(sh, sw), window=(top, left), a_stride=sa, b_stride=sb)
        assert got.cpu().tolist() == _want_sse(a, b, top, left, h, w, depth), (depth, h, w)
        # the access form changes no bit: the same frames packed and aligned
        packed = ops.yuv420_sse(_dev(_file_bytes(a)), _dev(_file_bytes(b)), 3, h, w, bps, src_hw=(sh, sw), window=(top, left))
        assert torch.equal(packed, got)
    with pytest.raises(ValueError, match="do not fit"):
        ops.yuv420_sse(ops_in[0], ops_in[1], 4, h, w, bps, src_hw=(sh, sw), a_stride=sa, b_stride=sb)


def test_yuv420_sse_sums_past_32_bits():
    """10 bit, 72 x 64: all 0 against all 1023 is 4608 * 1023^2 > 2^32 on the luma plane; a second, identical pair is 0."""
    from boosting_nerv_amd import ops
    h, w, peak = 72, 64, 1023
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    zero = tuple(np.zeros(s, dtype="<u2") for s in shapes)
    full = tuple(np.full(s, peak, dtype="<u2") for s in shapes)
    some = _planes(np.random.default_rng(71), 1, h, w, 10)[0]
    got = ops.yuv420_sse(_dev(_file_bytes([zero, some])), _dev(_file_bytes([full, some])), 2, h, w, 2).cpu().tolist()
    assert h * w == 4608 and 4608 * peak ** 2 > 2 ** 32
    assert got == [[4608 * peak ** 2, 1152 * peak ** 2, 1152 * peak ** 2], [0, 0, 0]]
    assert got[0] == _want_sse([zero], [full], 0, 0, h, w, 10)[0]


def test_yuv420_sse_refuses_what_it_cannot_do():
    from boosting_nerv_amd import ops
    from boosting_nerv_amd._lib import BnervError
    raw = torch.zeros(yuvio.frame_samples(18, 34), dtype=torch.uint8, device=DEV)
    small = torch.zeros(yuvio.frame_samples(16, 28), dtype=torch.uint8, device=DEV)
    with pytest.raises(BnervError, match="must be even"):
        ops.yuv420_sse(small, raw, 1, 16, 28, 1, src_hw=(18, 34), window=(1, 2))
    with pytest.raises(BnervError, match="leaves"):
        ops.yuv420_sse(small, raw, 1, 16, 28, 1, src_hw=(18, 34), window=(4, 2))
    with pytest.raises(ValueError, match="bytes_per_sample"):
        ops.yuv420_sse(small, raw, 1, 16, 28, 3, src_hw=(18, 34))
    with pytest.raises(ValueError, match="out must be"):
        ops.yuv420_sse(raw, raw, 1, 18, 34, 1, out=torch.zeros(1, 3, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- yuv_luma_f32
@pytest.mark.parametrize("depth", [8, 10])
def test_yuv_luma_f32_is_the_numpy_division_bit_for_bit(depth):
    from boosting_nerv_amd import ops
    gen = np.random.default_rng(81 + depth)
    bps, peak = _bps(depth), np.float32(2 ** depth - 1)
    for (h, w), src, (top, left) in SSE_SHAPES + [((13, 29), (18, 34), (3, 5))]:
        sh, sw = src or (h, w)
        frames = _planes(gen, 2, sh, sw, depth)
        stride = yuvio.frame_samples(sh, sw) * bps + 6
        got = ops.yuv_luma_f32(_dev(_file_bytes(frames, stride)), bps, 2, sh, sw, window=(top, left, h, w), frame_stride_bytes=stride)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 1, h, w)
        want = np.stack([f[0][top:top + h, left:left + w].astype(np.float32) / peak for f in frames])[:, None]
        assert want.dtype == np.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (depth, h, w, src, top, left)
    # every code of the depth, whole frame, into a view 4 bytes off its buffer
    codes = np.arange(2 ** depth, dtype=np.uint8 if depth == 8 else np.dtype("<u2"))
    h, w = 2 ** depth // 32, 32
    frame = (codes.reshape(h, w), codes[:h * w // 4].reshape(h // 2, w // 2), codes[:h * w // 4].reshape(h // 2, w // 2))
    ob = torch.full((h * w + 2,), float("nan"), device=DEV)
    out = ob[1:-1].view(1, 1, h, w)
    assert out.data_ptr() % 16 == 4
    ops.yuv_luma_f32(_dev(_file_bytes([frame])), bps, 1, h, w, out=out)
    assert np.array_equal(out.cpu().numpy().reshape(-1).view(np.uint32), (codes.astype(np.float32) / peak).view(np.uint32))
    assert torch.isnan(ob[0]).item() and torch.isnan(ob[-1]).item()


# ---------------------------------------------------------------------------------------------------------------------- MS-SSIM-Y
def _smooth_pair(depth, h, w, seed):
    """A smoothed random luma plane and its noisy copy as integer codes (chroma: mid grey)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.avg_pool2d(torch.rand(1, 1, h, w, generator=g), 3, stride=1, padding=1)
    y = (x + 0.08 * torch.randn(1, 1, h, w, generator=g)).clamp(0, 1)
    peak, dt = 2 ** depth - 1, np.uint8 if depth == 8 else np.dtype("<u2")
    grey = np.full((h // 2, w // 2), 2 ** (depth - 1), dtype=dt)
    return tuple((np.floor(t[0, 0].numpy().astype(np.float64) * peak + 0.5).astype(dt), grey, grey) for t in (x, y))


class _FixedFrames:
    """What Decoder.score needs of a decoder whose frame loop is a table of frames: score() itself is codec.Decoder's."""

    def __init__(self, f32, coeffs):
        from boosting_nerv_amd import codec, ops
        self.n_frames, self.frame_hw, self.device = f32.shape[0], tuple(f32.shape[-2:]), f32.device
        self.pack, self.coeffs = coeffs.pix_fmt, coeffs
        self._f32, self._packed = f32, ops.rgb_to_yuv420(f32, coeffs)
        self.score = codec.Decoder.score.__get__(self)
        self._need_pack = codec.Decoder._need_pack.__get__(self)

    def _launch(self, i):
        return self._f32[i:i + 1], self._packed[i:i + 1]


@pytest.mark.parametrize("depth", [8, 10])
def test_msssim_y_against_the_independent_form(tmp_path, depth):
    """162 x 178: ops.msssim on the two ops.yuv_luma_f32 planes within 2e-5 of tests/msssim_independent.py (the bound
    test_msssim_kernel_against_independent_form holds the kernel to) on the same quotients in float64."""
    import msssim_independent as ind
    from boosting_nerv_amd import ops
    h, w, bps, peak = 162, 178, _bps(depth), 2 ** depth - 1
    a, b = _smooth_pair(depth, h, w, 90 + depth)
    la = ops.yuv_luma_f32(_dev(_file_bytes([a])), bps, 1, h, w)
    lb = ops.yuv_luma_f32(_dev(_file_bytes([b])), bps, 1, h, w)
    got = ops.msssim(la, lb).double().cpu().numpy()
    want = ind.ms_ssim(a[0].astype(np.float64)[None, None] / peak, b[0].astype(np.float64)[None, None] / peak)
    print(f"  MS-SSIM-Y {depth} bit {h}x{w}: kernel {got}, independent {want}, |diff| {np.abs(got - want).max():.3g}")
    assert got.shape == want.shape == (1,) and 0.05 < want[0] < 0.999
    assert np.abs(got - want).max() < 2e-5


@pytest.mark.parametrize("depth", [8, 10])
def test_score_reports_none_for_msssim_at_160_rows(tmp_path, depth):
    """min(H, W) = 160 is below the five-scale MS-SSIM's limit: the MS-SSIM entries are None, nothing raises, the PSNR entries stand;
    at 162 x 178 the same call gives the MS-SSIM-Y of the two luma planes."""
    from boosting_nerv_amd import ops
    c = yuvio.coefficients("bt709", "limited", depth)
    for (h, w), has in (((160, 176), False), ((162, 178), True)):
        f32 = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(7)).to(DEV)
        frames = _planes(np.random.default_rng(95), 2, h, w, depth)
        path = tmp_path / f"src_{w}x{h}_{depth}bit.yuv"
        yuvio.write(path, frames, c.pix_fmt)
        dec = _FixedFrames(f32, c)
        got = dec.score(yuvio.YuvFile(path), rgb=True)
        packed = dec._packed.cpu().numpy().view(c.dtype)
        for i in range(2):
            hw, q = h * w, h * w // 4
            planes = (packed[i, :hw].reshape(h, w), packed[i, hw:hw + q].reshape(h // 2, w // 2), packed[i, hw + q:].reshape(h // 2, w // 2))
            one = yuvio.psnr_planes(planes, frames[i], depth)
            assert got["sse"][i].tolist() == [one["sse_y"], one["sse_u"], one["sse_v"]]
            assert [got[k][i] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv")] == [one[k] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv")]
        assert got["psnr_rgb"].shape == (2,) and np.isfinite(got["psnr_rgb"]).all()
        if not has:
            assert got["msssim_y"] is None and got["msssim_rgb"] is None and got["mean"]["msssim_y"] is None and got["mean"]["msssim_rgb"] is None
        else:
            src = _dev(_file_bytes(frames[1:2]))
            want = ops.msssim(ops.yuv_luma_f32(dec._packed[1], c.bytes_per_sample, 1, h, w), ops.yuv_luma_f32(src, c.bytes_per_sample, 1, h, w))
            assert got["msssim_y"].dtype == np.float32 and torch.equal(torch.from_numpy(got["msssim_y"][1:2]), want.cpu())
            assert got["msssim_rgb"].shape == (2,)
        off = dec.score(yuvio.YuvFile(path), msssim=False)
        assert off["msssim_y"] is None and "psnr_rgb" not in off and np.array_equal(off["sse"], got["sse"])


# ---------------------------------------------------------------------------------------------------------------------- Decoder.score
def _encoded(name):
    import test_gpu_codec as G                                # the tiny 180x320 bitstreams, built once per session
    return G._encoded(name), G.N_FRAMES, G.HW


_sources = {}


def _source(tmp_path_factory, depth, n, hw, margin=6):
    """The synthetic clip `margin` rows and columns larger than the decoded frames as a raw file, written once per depth."""
    if depth not in _sources:
        from boosting_nerv_amd import synth
        h, w = hw[0] + margin, hw[1] + margin
        video, c = synth.SyntheticVideo(n, h, w), yuvio.coefficients("bt709", "limited", depth)
        frames = [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(n)]
        path = tmp_path_factory.mktemp("score") / f"src_{w}x{h}_{depth}bit.yuv"
        yuvio.write(path, frames, yuvio.pix_fmt_of(depth))
        _sources[depth] = (str(path), frames)
    return _sources[depth]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", ["NeRV_Boost", "HNeRV_Boost"])
def test_decoder_score_equals_the_host_path(tmp_path_factory, name, depth, use_graph):
    """The source is 6 rows and columns larger than the clip: the centre crop's offset 3 is used as 2, as `codec psnr` does.  Exact
    integers, equal floats; the decoder decodes the same bytes afterwards."""
    from boosting_nerv_amd import codec, ops
    ref, n, (H, W) = _encoded(name)
    path, frames = _source(tmp_path_factory, depth, n, (H, W))
    clip = yuvio.YuvFile(path)
    assert yuvio.crop_offsets(clip.height, clip.width, H, W) == (3, 3)
    dec = codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=use_graph, pack=clip.pix_fmt)
    before = [dec.decode_yuv(i) for i in range(n)]
    got = dec.score(clip, chunk=3)                          # 4 frames in chunks of 3: both staging buffers
    assert got["sse"].dtype == np.int64 and got["sse"].shape == (n, 3)
    names = ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv")
    for i in range(n):
        one = yuvio.psnr_planes(dec.split_planes(before[i]), _window_of(frames[i], 2, 2, H, W), depth)
        assert got["sse"][i].tolist() == [one["sse_y"], one["sse_u"], one["sse_v"]], (name, depth, i)
        for k in names:
            assert got[k].dtype == np.float64 and got[k][i] == one[k], (name, depth, i, k)
    for k in names:
        assert got["mean"][k] == sum((float(v) for v in got[k]), 0.0) / n
    bps, raw = clip.bytes_per_sample, _dev(clip.raw(0, n))
    for i in range(n):                                      # MS-SSIM-Y: ops.msssim on the luma planes of the same two frames
        la = ops.yuv_luma_f32(_dev(before[i].view(np.uint8)), bps, 1, H, W)
        lb = ops.yuv_luma_f32(raw[i * clip.frame_bytes:(i + 1) * clip.frame_bytes], bps, 1, clip.height, clip.width, window=(2, 2, H, W))
        assert np.array_equal(got["msssim_y"][i:i + 1], ops.msssim(la, lb).cpu().numpy(), equal_nan=True), (name, depth, i)
    assert got["msssim_y"].dtype == np.float32 and got["msssim_y"].shape == (n,)
    assert "psnr_rgb" not in got
    assert np.array_equal(dec.decode_yuv(0), before[0])
    count = 0
    for i, frame in enumerate(dec):
        assert np.array_equal(frame, before[i])
        count += 1
    assert count == n
    again = dec.score(clip, msssim=False, chunk=1)
    assert np.array_equal(again["sse"], got["sse"]) and again["msssim_y"] is None


@pytest.mark.parametrize("depth", [8, 10])
def test_decoder_score_rgb_goes_through_the_loaders_kernels(tmp_path_factory, depth):
    """rgb=True: the source frame is the tensor training saw (YuvFile.to_device with the loader's window, odd offsets included), scored
    by the kernels evaluate() scores with -- the same bits."""
    from boosting_nerv_amd import codec, ops
    ref, n, (H, W) = _encoded("HNeRV_Boost")
    path, _ = _source(tmp_path_factory, depth, n, (H, W))
    src = yuvio.YuvFile(path)
    clip = src.to_device(DEV, crop=(H, W))
    dec = codec.Decoder(io.BytesIO(ref["blob"]), DEV, pack=src.pix_fmt)
    got = dec.score(src, rgb=True)
    for i in range(n):
        f32 = dec.decode_f32(i)
        assert torch.equal(torch.from_numpy(got["psnr_rgb"][i:i + 1]), ops.psnr(f32, clip[i:i + 1]).cpu()), (depth, i)
        assert torch.equal(torch.from_numpy(got["msssim_rgb"][i:i + 1]), ops.msssim(f32, clip[i:i + 1]).cpu()), (depth, i)
    for k in ("psnr_rgb", "msssim_rgb"):
        mean = torch.from_numpy(got[k]).to(DEV).sum().reshape(1).float() / float(n)          # runtime.MetricBook.means
        assert got["mean"][k] == mean.item()


def test_decoder_score_refusals(tmp_path_factory):
    from boosting_nerv_amd import codec
    ref, n, (H, W) = _encoded("NeRV_Boost")
    path, frames = _source(tmp_path_factory, 8, n, (H, W))
    clip = yuvio.YuvFile(path)
    with pytest.raises(RuntimeError, match="packs rgb8"):
        codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=False, pack="rgb8").score(clip)
    with pytest.raises(RuntimeError, match="yuv420p10le"):
        codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=False, pack="yuv420p10le").score(clip)
    short = tmp_path_factory.mktemp("short") / f"short_{clip.width}x{clip.height}_8bit.yuv"
    yuvio.write(short, frames[:n - 1], "yuv420p")
    with pytest.raises(ValueError, match="frames"):
        codec.Decoder(io.BytesIO(ref["blob"]), DEV, use_graph=False, pack="yuv420p").score(yuvio.YuvFile(short))


# ---------------------------------------------------------------------------------------------------------------------- command line
POSTHOC_LINE = ("--outf t --vid tiny --model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --crop_list 180_320 "
                "--resize_list -1 --loss L2 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 --modelsize 0.05 "
                "--lower_width 6 -b 1 --lr 0.001 --eval_freq 1 -p 2 -e 1 --not_resume")
CEM_LINE = ("--outf t --vid tiny --model HNeRV_Boost --sft_block res_sft --ch_t 32 --optim_type Adan --conv_type convnext pshuffel_3x3 --act sin "
            "--norm none --crop_list 180_320 --resize_list -1 --loss Fusion10_freq --embed pe_1.25_80 --enc_strds 5 2 2 --enc_dim 16_4 --dec_strds 5 2 2 "
            "--ks 0_1_5 --reduce 1.2 --dec_blks 1 1 2 --modelsize 0.05 --lower_width 6 -b 1 -e 2 --eval_freq 2 --lr 0.002 --lr_type cosine_0_1_0.1 "
            "--not_resume --embed_entropy --quant --quant_model_bit 8 --quant_bias_bit 8 --quant_embed_bit 8 --quantizer_w scale --quantizer_b scale "
            "--quantizer_e scalebeta --lambda_rate 0.5 --target_bit 2 -p 1")


@pytest.mark.isolated
@pytest.mark.parametrize("kind", ["posthoc", "cem"])
def test_cli_score_on_a_file_the_train_script_wrote_from_a_raw_clip(tmp_path, monkeypatch, capsys, kind):
    """The README's 4-frame tiny recipes on the synthetic clip stored as a raw file: `codec score` prints the integers and the four PSNR
    floats `codec psnr` prints, --rgb gives per frame what the run's quant_seen_psnr averages, --per_frame writes 4 rows."""
    from boosting_nerv_amd import codec, ops, synth
    from boosting_nerv_amd import train_nerv_all as T, train_nerv_compression as TC
    monkeypatch.chdir(tmp_path)
    c = yuvio.coefficients("bt709", "limited", 8)
    video = synth.SyntheticVideo(4, 180, 320)
    src = tmp_path / "clip_320x180_8bit.yuv"
    yuvio.write(src, [yuvio.to_yuv_reference(video.frame(i).numpy(), c) for i in range(4)], c.pix_fmt)
    mod, line, stream = (T, POSTHOC_LINE, tmp_path / "tiny.bnrq") if kind == "posthoc" else (TC, CEM_LINE, tmp_path / "tiny.bnrv")
    seen = {}
    orig_eval = mod.evaluate

    def spy(model, loader, rank, args, *a, **k):
        out = orig_eval(model, loader, rank, args, *a, **k)
        seen["clip"], seen["results"] = args._frames_dev.clone(), out[0]
        return out
    monkeypatch.setattr(mod, "evaluate", spy)
    mod.main((line + f" --data_path {src} --bitstream {stream}").split())
    capsys.readouterr()
    csv_path = tmp_path / "frames.csv"
    scored = codec.main(["score", str(stream), "--ref", str(src), "--rgb", "--per_frame", str(csv_path)])
    out = capsys.readouterr().out.strip().splitlines()
    assert "PSNR-YUV" in out[-2] and "MSSSIM-Y" in out[-2] and "PSNR-RGB" in out[-2] and json.loads(out[-1]) == scored
    host = codec.main(["psnr", str(stream), "--ref", str(src)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for k in ("sse_y", "sse_u", "sse_v", "psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "frames", "pix_fmt", "matrix", "range"):
        assert scored[k] == host[k] == printed[k], k
    assert isinstance(scored["sse_y"], int) and scored["sse_y"] > 0 and 0.0 < scored["msssim_y"] < 1.0
    dec = codec.Decoder(str(stream), DEV)
    want = [ops.psnr(dec.decode_f32(i), seen["clip"][i:i + 1]) for i in range(4)]
    with open(csv_path) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4 and [int(r["frame"]) for r in rows] == [0, 1, 2, 3]
    assert sum(int(r["sse_y"]) for r in rows) == scored["sse_y"]
    for r, w in zip(rows, want):
        assert np.float32(float(r["psnr_rgb"])) == w.cpu().numpy()[0]
    mean = torch.cat(want).sum().reshape(1).float() / 4.0                                   # runtime.MetricBook.means
    assert scored["psnr_rgb"] == mean.item()
    assert torch.equal(mean.cpu(), seen["results"][4])                                       # the quant_seen_psnr of the run's last evaluation
    ssim = torch.cat([ops.msssim(dec.decode_f32(i), seen["clip"][i:i + 1]) for i in range(4)]).sum().reshape(1).float() / 4.0
    assert scored["msssim_rgb"] == ssim.item() and torch.equal(ssim.cpu(), seen["results"][5])  # and its quant_seen_ssim
    with pytest.raises(RuntimeError, match="packs rgb8"):
        dec.score(yuvio.YuvFile(src))
