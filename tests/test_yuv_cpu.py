"""Raw YUV 4:2:0 video in and out, the parts that need no GPU: the float64 restatement against values worked out by
hand, the file reader and writer, per-plane PSNR, the new flags, and the argument validation of the two entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from boosting_nerv_amd import yuvio


def _flat(coeffs, y, u, v, h=2, w=2):
    return yuvio.to_rgb_reference(np.full((h, w), y), np.full((h // 2, w // 2), u), np.full((h // 2, w // 2), v), coeffs)


# ---------------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("depth", [8, 10])
def test_limited_range_bt709_anchors(depth):
    """Reference white, reference black and the bt709 red primary, by hand: (63, 102, 240) is Y' = 47/219, Cb' = -26/224, Cr' = 112/224, i.e.
    R = 0.2146 + 1.5748 * 0.5 = 1.0020, G = 0.2146 + 0.1873 * 0.1161 - 0.4681 * 0.5 = 0.0023, B = 0.2146 - 1.8556 * 0.1161 = -0.0008 -- red
    within one luma code (1/219) per channel.  At 10 bit the codes are four times as large and mean the same."""
    s = 2 ** (depth - 8)
    c = yuvio.coefficients("bt709", "limited", depth)
    assert c.pix_fmt == ("yuv420p" if depth == 8 else "yuv420p10le") and c.bytes_per_sample == (1 if depth == 8 else 2)
    white, black, red = _flat(c, 235 * s, 128 * s, 128 * s), _flat(c, 16 * s, 128 * s, 128 * s), _flat(c, 63 * s, 102 * s, 240 * s)
    assert white.shape == (3, 2, 2) and white.dtype == np.float64
    assert np.abs(white - 1.0).max() < 1e-12 and np.abs(black).max() < 1e-12
    assert np.abs(red - np.array([1.0, 0.0, 0.0]).reshape(3, 1, 1)).max() < 1.0 / 219


def test_full_range_white_and_out_of_range_codes_are_clamped():
    c = yuvio.coefficients("bt709", "full", 8)
    # chroma 128 is half a code above the centre 127.5 of the full range: (128 - 128) / 255 = 0 here, so white is exact; one code off is < 0.5 / 255 * 1.86
    assert np.abs(_flat(c, 255, 128, 128) - 1.0).max() < 0.5 / 255
    assert np.abs(_flat(c, 255, 127, 127) - 1.0).max() < 1.86 / 255
    lim = yuvio.coefficients("bt709", "limited", 8)
    assert _flat(lim, 255, 128, 128).max() == 1.0 and _flat(lim, 0, 128, 128).min() == 0.0     # super-white / sub-black


def test_matrix_constants():
    for name, (kr, kb) in (("bt709", (0.2126, 0.0722)), ("bt601", (0.299, 0.114))):
        c = yuvio.coefficients(name, "full", 8)
        kg = 1 - kr - kb
        np.testing.assert_allclose(c.to_yuv[0], [kr, kg, kb], rtol=0, atol=1e-15)
        np.testing.assert_allclose(c.to_rgb[:, 2], [2 * (1 - kr), -2 * kr * (1 - kr) / kg, 0.0], rtol=0, atol=1e-15)
        np.testing.assert_allclose(c.to_rgb[:, 1], [0.0, -2 * kb * (1 - kb) / kg, 2 * (1 - kb)], rtol=0, atol=1e-15)
        np.testing.assert_allclose(c.to_rgb @ c.to_yuv, np.eye(3), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="matrix"):
        yuvio.coefficients("bt2020", "limited", 8)
    with pytest.raises(ValueError, match="range"):
        yuvio.coefficients("bt709", "tv", 8)
    with pytest.raises(ValueError, match="depth"):
        yuvio.coefficients("bt709", "limited", 12)
    s = yuvio.coefficients("bt709", "limited", 10).load_struct()
    assert s.maxcode == 1023.0 and s.off[0] == 64.0 and s.scale[1] == np.float32(1.0 / 896.0) and s.m[2] == np.float32(1.5748)


# ---------------------------------------------------------------------------------------------------------------------- siting
def _upsampled_chroma(u, v, h, w, crop=None):
    """The up-sampled chroma planes, read back through a full-range bt709 conversion of a black luma plane:
    B = 2 (1 - Kb) (U - 128) / 255 and R = 2 (1 - Kr) (V - 128) / 255 (the codes below keep both inside [0, 1])."""
    c = yuvio.coefficients("bt709", "full", 8)
    rgb = yuvio.to_rgb_reference(np.zeros((h, w), np.uint8), u, v, c, crop)
    return rgb[2] * 255 / (2 * (1 - 0.0722)) + 128, rgb[0] * 255 / (2 * (1 - 0.2126)) + 128


U46 = np.array([[130, 150, 190], [170, 210, 250]], dtype=np.uint8)
# rows: C[0];  3/4 C[0] + 1/4 C[1];  3/4 C[1] + 1/4 C[0];  C[1].   columns: c0, (c0 + c1) / 2, c1, (c1 + c2) / 2, c2, c2 (right edge clamped)
UP46 = np.array([[130, 140, 150, 170, 190, 190],
                 [140, 152.5, 165, 185, 205, 205],
                 [160, 177.5, 195, 215, 235, 235],
                 [170, 190, 210, 230, 250, 250]])


def test_upsampling_siting_with_clamped_edges():
    u, v = _upsampled_chroma(np.array([[200]], np.uint8), np.array([[131]], np.uint8), 2, 2)
    assert np.abs(u - 200).max() < 1e-9 and np.abs(v - 131).max() < 1e-9            # one chroma sample: every edge is clamped
    u, v = _upsampled_chroma(U46, U46[::-1], 4, 6)
    assert np.abs(u - UP46).max() < 1e-9 and np.abs(v - UP46[::-1]).max() < 1e-9
    # a crop at odd offsets is a window of the same picture: the formulas run on source coordinates
    u, v = _upsampled_chroma(U46, U46[::-1], 4, 6, crop=(1, 1, 2, 3))
    assert np.abs(u - UP46[1:3, 1:4]).max() < 1e-9 and np.abs(v - UP46[::-1][1:3, 1:4]).max() < 1e-9
    with pytest.raises(ValueError, match="crop"):
        _upsampled_chroma(U46, U46, 4, 6, crop=(1, 1, 4, 3))


def test_downsampling_siting_with_clamped_left_edge():
    """Full range bt709, a frame with G = B = 0: Y = floor(255 Kr R + 0.5), Cr' = R / 2, Cb' = -Kr R / (2 (1 - Kb)), both filtered.
    R along a row is (0, 1/2, 1, 1/2, 0, 1): [1 2 1] / 4 at x = 0 (left edge clamped), 2, 4 gives 1/8, 3/4, 3/8 -- rows 2 and 3 carry it, of
    rows 0 and 1 only row 0 does, so the first chroma row sees half of it."""
    row = np.array([0, 0.5, 1, 0.5, 0, 1])
    rgb = np.zeros((3, 4, 6))
    rgb[0, 0], rgb[0, 2], rgb[0, 3] = row, row, row
    y, u, v = yuvio.to_yuv_reference(rgb, yuvio.coefficients("bt709", "full", 8))
    yrow = [0, 27, 54, 27, 0, 54]                               # 255 * 0.2126 = 54.213
    assert y.dtype == np.uint8 and y.tolist() == [yrow, [0] * 6, yrow, yrow]
    # 128.5 + 127.5 * (1/16, 3/8, 3/16) = 136.47, 176.31, 152.41;  128.5 + 127.5 * (1/8, 3/4, 3/8) = 144.44, 224.13, 176.31
    assert v.tolist() == [[136, 176, 152], [144, 224, 176]]
    # 255 * -0.2126 / 1.8556 = -29.216:  128.5 - 29.216 * (1/16, 3/8, 3/16) = 126.67, 117.54, 123.02;  * (1/8, 3/4, 3/8): 124.85, 106.59, 117.54
    assert u.tolist() == [[126, 117, 123], [124, 106, 117]]
    hot = yuvio.to_yuv_reference(np.full((3, 2, 2), 7.0), yuvio.coefficients("bt709", "limited", 10))        # out of range: clamped to white
    assert [p.dtype for p in hot] == [np.dtype("<u2")] * 3 and [int(p[0, 0]) for p in hot] == [940, 512, 512]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("rng_name", ["limited", "full"])
def test_flat_colours_survive_the_round_trip_within_one_code(depth, matrix, rng_name):
    c = yuvio.coefficients(matrix, rng_name, depth)
    s = 2 ** (depth - 8)
    for code in [(16, 128, 128), (235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (120, 100, 150), (200, 128, 128)]:
        code = tuple(k * s for k in code)
        rgb = yuvio.to_rgb_reference(np.full((4, 6), code[0]), np.full((2, 3), code[1]), np.full((2, 3), code[2]), c)
        if rgb.min() <= 0.0 or rgb.max() >= 1.0:                # outside the RGB cube: the clamp loses it by design
            continue
        back = yuvio.to_yuv_reference(rgb, c)
        for plane, k in zip(back, code):
            assert np.abs(plane.astype(np.int64) - k).max() <= 1, (code, plane)


# ---------------------------------------------------------------------------------------------------------------------- files
def _random_planes(gen, h, w, depth):
    top = 2 ** depth
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    return tuple(gen.integers(0, top, shape).astype(dt) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def test_yuvfile_reads_what_write_wrote(tmp_path):
    gen = np.random.default_rng(3)
    frames = [_random_planes(gen, 4, 6, 8) for _ in range(3)]
    path = tmp_path / "clip_6x4_8bit.yuv"
    assert yuvio.write(path, frames, "yuv420p") == 3
    assert os.path.getsize(path) == 3 * 36
    clip = yuvio.YuvFile(path)
    assert (len(clip), clip.width, clip.height, clip.pix_fmt, clip.depth, clip.frame_bytes) == (3, 6, 4, "yuv420p", 8, 36)
    for i, f in enumerate(frames):
        for got, want in zip(clip.planes(i), f):
            assert got.dtype == np.uint8 and np.array_equal(got, want)
    with pytest.raises(IndexError):
        clip.planes(3)
    # the raw bytes are the planes in order, and a frame in file layout (what the decoder yields) is written as it stands
    assert bytes(clip.raw(1, 2)) == b"".join(p.tobytes() for p in frames[1])
    again = tmp_path / "again_6x4_8bit.yuv"
    yuvio.write(again, [np.concatenate([p.reshape(-1) for p in f]) for f in frames], "yuv420p")
    assert again.read_bytes() == path.read_bytes()
    rgb = clip.frame_rgb(1, crop=(2, 4))
    top, left = yuvio.crop_offsets(4, 6, 2, 4)
    assert (top, left) == (1, 1) and rgb.dtype == np.float32 and rgb.shape == (3, 2, 4)
    want = yuvio.to_rgb_reference(*frames[1], yuvio.coefficients("bt709", "limited", 8), (1, 1, 2, 4))
    assert np.array_equal(rgb, want.astype(np.float32))


def test_yuvfile_ten_bit_is_little_endian(tmp_path):
    gen = np.random.default_rng(4)
    frame = _random_planes(gen, 2, 4, 10)
    frame[0][0, 0] = 0x0302                                       # bytes 02 03 in the file
    path = tmp_path / "Beauty_4x2_120fps_420_10bit_YUV.yuv"
    yuvio.write(path, [frame], "yuv420p10le")
    data = path.read_bytes()
    assert len(data) == 12 * 2 and data[0] == 0x02 and data[1] == 0x03
    clip = yuvio.YuvFile(path)
    assert (len(clip), clip.width, clip.height, clip.pix_fmt, clip.bytes_per_sample) == (1, 4, 2, "yuv420p10le", 2)
    assert all(np.array_equal(a, b) for a, b in zip(clip.planes(0), frame)) and int(clip.planes(0)[0][0, 0]) == 770
    with pytest.raises(ValueError, match="0..1023"):
        yuvio.write(tmp_path / "bad.yuv", [(np.full((2, 2), 1024), np.zeros((1, 1), int), np.zeros((1, 1), int))], "yuv420p10le")


def test_yuvfile_name_parsing_and_errors(tmp_path):
    assert yuvio.parse_name("/data/Beauty_1920x1080_120fps_420_8bit_YUV.yuv") == (1920, 1080, "yuv420p")
    assert yuvio.parse_name("ReadySteadyGo_3840x2160_120fps_420_10bit_YUV.yuv") == (3840, 2160, "yuv420p10le")
    assert yuvio.parse_name("clip.yuv") == (None, None, None)
    raw = tmp_path / "clip.yuv"
    raw.write_bytes(bytes(36))
    with pytest.raises(ValueError, match="--yuv_size"):
        yuvio.YuvFile(raw)
    with pytest.raises(ValueError, match="--yuv_fmt"):
        yuvio.YuvFile(raw, 6, 4)
    assert len(yuvio.YuvFile(raw, 6, 4, "yuv420p")) == 1           # arguments stand in for the name
    with pytest.raises(ValueError, match="whole number"):
        yuvio.YuvFile(raw, 6, 4, "yuv420p10le")                     # 36 bytes are half a 10-bit frame
    with pytest.raises(ValueError, match="even"):
        yuvio.YuvFile(raw, 3, 8, "yuv420p")
    with pytest.raises(ValueError, match="pixel format"):
        yuvio.YuvFile(raw, 6, 4, "yuv422p")
    named = tmp_path / "clip_6x4_8bit.yuv"
    named.write_bytes(bytes(36 + 5))
    with pytest.raises(ValueError, match="whole number"):
        yuvio.YuvFile(named)
    with pytest.raises(ValueError, match="WIDTHxHEIGHT"):
        yuvio.parse_size("6*4")
    with pytest.raises(NotImplementedError, match="smaller"):
        yuvio.YuvFile(raw, 6, 4, "yuv420p").frame_rgb(0, crop=(6, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        yuvio.YuvFile(raw, 6, 4, "yuv420p").to_device("cpu")


def test_psnr_planes_against_numpy():
    gen = np.random.default_rng(5)
    for depth in (8, 10):
        a, b = _random_planes(gen, 6, 8, depth), _random_planes(gen, 6, 8, depth)
        got = yuvio.psnr_planes(a, b, depth)
        peak = 2 ** depth - 1
        want = []
        for name, pa, pb in zip("yuv", a, b):
            sse = sum((int(x) - int(y)) ** 2 for x, y in zip(pa.reshape(-1).tolist(), pb.reshape(-1).tolist()))
            assert got[f"sse_{name}"] == sse and isinstance(got[f"sse_{name}"], int)
            want.append(10 * np.log10(peak ** 2 / np.mean((pa.astype(np.float64) - pb.astype(np.float64)) ** 2)))
            assert abs(got[f"psnr_{name}"] - want[-1]) < 1e-9
        assert abs(got["psnr_yuv"] - (6 * want[0] + want[1] + want[2]) / 8) < 1e-9
        same = yuvio.psnr_planes(a, a, depth)
        assert same["sse_y"] == same["sse_u"] == same["sse_v"] == 0 and same["psnr_y"] == same["psnr_yuv"] == float("inf")
    with pytest.raises(ValueError, match="plane u"):
        yuvio.psnr_planes(a, (a[0], a[1][:1], a[2]), 10)


# ---------------------------------------------------------------------------------------------------------------------- flags
def test_train_parsers_take_the_yuv_flags():
    from boosting_nerv_amd import train_nerv_all as T, train_nerv_compression as TC
    for mod in (T, TC):
        a = mod.build_parser().parse_args([])
        assert (a.yuv_size, a.yuv_fmt, a.yuv_matrix, a.yuv_range) == (None, None, "bt709", "limited")
        a = mod.build_parser().parse_args("--data_path x.yuv --yuv_size 320x180 --yuv_fmt yuv420p10le --yuv_matrix bt601 --yuv_range full".split())
        assert (a.yuv_size, a.yuv_fmt, a.yuv_matrix, a.yuv_range) == ("320x180", "yuv420p10le", "bt601", "full")
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--yuv_fmt", "yuv444p"])


def test_codec_parser_takes_the_yuv_format_and_psnr():
    from boosting_nerv_amd import codec
    p = codec.build_parser()
    a = p.parse_args("decode f.bnrv --out clip.yuv --format yuv".split())
    assert (a.cmd, a.format, a.pix_fmt, a.matrix, a.range) == ("decode", "yuv", "yuv420p", "bt709", "limited")
    a = p.parse_args("decode f.bnrv --out clip.yuv --format yuv --pix_fmt yuv420p10le --matrix bt601 --range full".split())
    assert (a.pix_fmt, a.matrix, a.range) == ("yuv420p10le", "bt601", "full")
    a = p.parse_args("psnr f.bnrv --ref src_320x180_8bit.yuv".split())
    assert (a.cmd, a.ref, a.size, a.pix_fmt, a.matrix, a.range) == ("psnr", "src_320x180_8bit.yuv", None, None, "bt709", "limited")
    a = p.parse_args("psnr f.bnrv --ref src.yuv --size 320x180 --pix_fmt yuv420p10le".split())
    assert (a.size, a.pix_fmt) == ("320x180", "yuv420p10le")
    assert p.parse_args("decode f.bnrv --out d".split()).format == "png"          # the default stands
    with pytest.raises(SystemExit):
        p.parse_args("psnr f.bnrv".split())


def test_dataset_serves_a_raw_clip_with_the_png_contract(tmp_path):
    """VideoDataSet on a .yuv path: the samples of the PNG path ('img' fp32 [3, h, w] in [0, 1], 'idx', 'norm_idx'), the centre crop, the
    interpolation recipes' drop of an even last frame and the neighbours of --embed_inter."""
    import torch
    from types import SimpleNamespace
    from boosting_nerv_amd.hnerv_utils import VideoDataSet
    gen = np.random.default_rng(6)
    frames = [_random_planes(gen, 8, 12, 8) for _ in range(4)]
    path = tmp_path / "clip_12x8_8bit.yuv"
    yuvio.write(path, frames, "yuv420p")
    ds = VideoDataSet(SimpleNamespace(data_path=str(path), crop_list="6_10"))
    assert len(ds) == 4 and ds.final_size == 60
    c = yuvio.coefficients("bt709", "limited", 8)
    s = ds[2]
    assert s["idx"] == 2 and s["norm_idx"] == 3 / 4 and s["img"].dtype == torch.float32 and tuple(s["img"].shape) == (3, 6, 10)
    assert np.array_equal(s["img"].numpy(), yuvio.to_rgb_reference(*frames[2], c, (1, 1, 6, 10)).astype(np.float32))
    assert 0.0 <= float(s["img"].min()) and float(s["img"].max()) <= 1.0
    other = VideoDataSet(SimpleNamespace(data_path=str(path), crop_list="8_12", yuv_matrix="bt601", yuv_range="full"))
    assert np.array_equal(other[0]["img"].numpy(), yuvio.to_rgb_reference(*frames[0], yuvio.coefficients("bt601", "full", 8)).astype(np.float32))
    inter = VideoDataSet(SimpleNamespace(data_path=str(path), crop_list="8_12", interpolation=True, embed_inter=True))
    assert len(inter) == 3
    s = inter[1]
    assert torch.equal(s["pre_img"], inter[0]["img"]) and torch.equal(s["post_img"], inter[2]["img"]) and s["norm_idx"] == 2 / 3
    with pytest.raises(NotImplementedError, match="smaller"):
        VideoDataSet(SimpleNamespace(data_path=str(path), crop_list="10_12"))
    bare = tmp_path / "bare.yuv"
    bare.write_bytes(path.read_bytes())
    with pytest.raises(ValueError, match="--yuv_size"):
        VideoDataSet(SimpleNamespace(data_path=str(bare), crop_list="8_12"))
    assert len(VideoDataSet(SimpleNamespace(data_path=str(bare), crop_list="8_12", yuv_size="12x8", yuv_fmt="yuv420p"))) == 4


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_validate_before_any_launch():
    """Every rejected argument returns BNERV_E_ARG (-1) with a message, with no GPU in the machine."""
    from boosting_nerv_amd import _lib as L, ops
    lib = L.load()
    assert lib.bnerv_abi_version() == 9
    assert callable(ops.yuv420_to_rgb) and callable(ops.rgb_to_yuv420)
    k = yuvio.coefficients("bt709", "limited", 8).load_struct()
    kp, one = C.byref(k), C.c_void_p(64)

    def load(src=one, bps=1, B=1, stride=6, h=2, w=2, top=0, left=0, out=one, ch=2, cw=2, coeffs=kp):
        return lib.bnerv_yuv420_to_rgb(None, src, bps, B, stride, h, w, top, left, out, ch, cw, coeffs)

    def store(x=one, B=1, h=2, w=2, out=one, bps=1, stride=6, coeffs=kp):
        return lib.bnerv_rgb_to_yuv420(None, x, B, h, w, out, bps, stride, coeffs)

    for bad in (dict(src=None), dict(out=None), dict(coeffs=None)):
        assert load(**bad) == -1 and b"yuv420_to_rgb: null" in lib.bnerv_last_error()
    for bad in (dict(h=3), dict(w=3, stride=9)):
        assert load(**bad) == -1 and b"even" in lib.bnerv_last_error()
    for bps in (0, 3, 4):
        assert load(bps=bps) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    for bad in (dict(top=1), dict(left=1), dict(ch=3), dict(cw=4), dict(top=-1), dict(left=-2, cw=1), dict(ch=0), dict(cw=0), dict(top=2 ** 31 - 1)):
        assert load(**bad) == -1 and b"crop" in lib.bnerv_last_error(), bad
    assert load(stride=5) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert load(bps=2, stride=11) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert load(bps=2, stride=13) == -1 and b"odd" in lib.bnerv_last_error()
    assert load(bps=2, stride=12, src=C.c_void_p(65)) == -1 and b"odd" in lib.bnerv_last_error()
    assert load(out=C.c_void_p(66)) == -1 and b"4-byte" in lib.bnerv_last_error()
    for bad in (dict(B=0), dict(B=70000), dict(h=0), dict(w=0)):
        assert load(**bad) == -1

    for bad in (dict(x=None), dict(out=None), dict(coeffs=None)):
        assert store(**bad) == -1 and b"rgb_to_yuv420: null" in lib.bnerv_last_error()
    for bad in (dict(h=3), dict(w=5, stride=15)):
        assert store(**bad) == -1 and b"even" in lib.bnerv_last_error()
    assert store(bps=3) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    assert store(stride=5) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert store(bps=2, stride=12, out=C.c_void_p(65)) == -1 and b"odd" in lib.bnerv_last_error()
    assert store(x=C.c_void_p(66)) == -1 and b"4-byte" in lib.bnerv_last_error()
    for bad in (dict(B=0), dict(B=70000), dict(h=0)):
        assert store(**bad) == -1
