"""The host side of `codec score`: the PSNR formula factored out of yuvio.psnr_planes, the command line's flags and the
refusals that need no GPU.  The device side is tests/test_gpu_score.py."""
import numpy as np
import pytest
import torch

from boosting_nerv_amd import yuvio


def _random_planes(gen, h, w, depth):
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    return tuple(gen.integers(0, 2 ** depth, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _psnr_planes_before(a, b, depth):
    """yuvio.psnr_planes as it stood before the formula moved to psnr_from_sse, line for line."""
    peak = 2 ** int(depth) - 1
    out = {}
    for name, pa, pb in zip("yuv", a, b):
        pa, pb = np.asarray(pa), np.asarray(pb)
        d = pa.astype(np.int64) - pb.astype(np.int64)
        sse = int((d * d).sum())
        out[f"sse_{name}"] = sse
        out[f"psnr_{name}"] = float("inf") if sse == 0 else 10.0 * float(np.log10(peak * peak * pa.size / sse))
    out["psnr_yuv"] = (6.0 * out["psnr_y"] + out["psnr_u"] + out["psnr_v"]) / 8.0
    return out


@pytest.mark.parametrize("depth", [8, 10])
def test_psnr_from_sse_reproduces_psnr_planes_bit_for_bit(depth):
    gen = np.random.default_rng(41 + depth)
    for h, w in ((2, 2), (6, 8), (18, 34), (64, 96)):
        a, b = _random_planes(gen, h, w, depth), _random_planes(gen, h, w, depth)
        want = yuvio.psnr_planes(a, b, depth)
        got = yuvio.psnr_from_sse([want["sse_y"], want["sse_u"], want["sse_v"]], h * w, depth)
        assert sorted(got) == ["psnr_u", "psnr_v", "psnr_y", "psnr_yuv"]
        for k, v in got.items():
            assert isinstance(v, float) and v == want[k] and np.isfinite(v), (h, w, k)
        # numpy integers (a row of the device's table) are taken as exact integers too
        assert yuvio.psnr_from_sse(np.array([want["sse_y"], want["sse_u"], want["sse_v"]], dtype=np.int64), h * w, depth) == got
        before = _psnr_planes_before(a, b, depth)
        assert want == before and list(want) == list(before)           # psnr_planes returns exactly what it returned before
    # a plane without error: inf there, and in the weighted mean
    one = yuvio.psnr_from_sse([0, 5, 7], 64, depth)
    assert one["psnr_y"] == float("inf") and np.isfinite(one["psnr_u"]) and np.isfinite(one["psnr_v"]) and one["psnr_yuv"] == float("inf")
    zero = yuvio.psnr_from_sse([0, 0, 0], 64, depth)
    assert all(v == float("inf") for v in zero.values())
    same = yuvio.psnr_planes(a, a, depth)
    assert {k: same[k] for k in zero} == zero


def test_psnr_from_sse_takes_sums_above_2_to_the_32():
    sse = 4608 * 1023 ** 2
    assert sse > 2 ** 32
    got = yuvio.psnr_from_sse([sse, sse // 4, 0], 4608, 10)
    assert got["psnr_y"] == got["psnr_u"] == 0.0 and got["psnr_v"] == float("inf")


def test_codec_parser_takes_score_and_its_flags():
    from boosting_nerv_amd import codec
    p = codec.build_parser()
    a = p.parse_args("score f.bnrq --ref clip.yuv".split())
    assert (a.cmd, a.file, a.ref, a.size, a.pix_fmt, a.matrix, a.range) == ("score", "f.bnrq", "clip.yuv", None, None, "bt709", "limited")
    assert (a.rgb, a.no_msssim, a.per_frame, a.no_graph) == (False, False, None, False)
    a = p.parse_args("score f.bnrz --ref clip.yuv --size 320x180 --pix_fmt yuv420p10le --matrix bt601 --range full --rgb --no_msssim "
                     "--per_frame out.csv --no_graph".split())
    assert (a.size, a.pix_fmt, a.matrix, a.range, a.rgb, a.no_msssim, a.per_frame, a.no_graph) == ("320x180", "yuv420p10le", "bt601", "full", True, True,
                                                                                                  "out.csv", True)
    with pytest.raises(SystemExit):
        p.parse_args("score f.bnrv".split())                        # --ref is required
    with pytest.raises(SystemExit):
        p.parse_args("score f.bnrv --ref clip.yuv --pix_fmt yuv444p".split())
    # the psnr command is as it was
    q = p.parse_args("psnr f.bnrv --ref clip.yuv".split())
    assert (q.cmd, q.size, q.pix_fmt, q.no_graph) == ("psnr", None, None, False) and not hasattr(q, "rgb")


def test_codec_score_without_a_gpu_raises_what_decode_raises(tmp_path, monkeypatch):
    from boosting_nerv_amd import codec
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no ROCm GPU") as scored:
        codec.main(["score", str(tmp_path / "none.bnrv"), "--ref", str(tmp_path / "none.yuv")])
    with pytest.raises(RuntimeError, match="no ROCm GPU") as decoded:
        codec.main(["decode", str(tmp_path / "none.bnrv"), "--out", str(tmp_path / "frames")])
    assert str(scored.value) == str(decoded.value)


def test_score_ops_refuse_host_tensors():
    from boosting_nerv_amd import ops
    from boosting_nerv_amd._lib import BnervError
    raw = torch.zeros(6, dtype=torch.uint8)
    with pytest.raises(BnervError, match="ROCm GPU"):
        ops.yuv420_sse(raw, raw, 1, 2, 2, 1)
    with pytest.raises(BnervError, match="ROCm GPU"):
        ops.yuv_luma_f32(raw, 1, 1, 2, 2)


def test_score_entry_points_validate_before_any_launch():
    """Every rejected argument returns BNERV_E_ARG (-1) with a message, with no GPU in the machine."""
    import ctypes as C
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    assert lib.bnerv_abi_version() == 9
    one = C.c_void_p(64)

    def sse(a=one, sa=6, b=one, sb=24, bps=1, B=1, h=2, w=2, sh=4, sw=4, top=0, left=0, out=one):
        return lib.bnerv_yuv420_sse(None, a, sa, b, sb, bps, B, h, w, sh, sw, top, left, out)

    def luma(src=one, bps=1, B=1, stride=24, sh=4, sw=4, top=0, left=0, out=one, h=2, w=2, maxcode=255.0):
        return lib.bnerv_yuv_luma_f32(None, src, bps, B, stride, sh, sw, top, left, out, h, w, maxcode)

    for bad in (dict(a=None), dict(b=None), dict(out=None)):
        assert sse(**bad) == -1 and b"yuv420_sse: null" in lib.bnerv_last_error()
    for bad in (dict(h=3), dict(w=3, sa=9), dict(sh=5, sb=30), dict(sw=3, sb=18)):
        assert sse(**bad) == -1 and b"even" in lib.bnerv_last_error(), bad
    for bps in (0, 3, 4):
        assert sse(bps=bps) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    for bad in (dict(top=1), dict(left=1), dict(top=-2), dict(left=-2)):
        assert sse(**bad) == -1 and b"must be even" in lib.bnerv_last_error(), bad
    for bad in (dict(top=4), dict(left=4), dict(h=6, sa=18), dict(w=6, sa=18), dict(top=2 ** 31 - 2)):
        assert sse(**bad) == -1 and b"leaves" in lib.bnerv_last_error(), bad
    assert sse(sa=5) == -1 and b"a: frame_stride_bytes" in lib.bnerv_last_error()
    assert sse(sb=23) == -1 and b"b: frame_stride_bytes" in lib.bnerv_last_error()
    assert sse(bps=2, sa=12, sb=49) == -1 and b"odd" in lib.bnerv_last_error()
    assert sse(bps=2, sa=12, sb=48, a=C.c_void_p(65)) == -1 and b"odd" in lib.bnerv_last_error()
    assert sse(out=C.c_void_p(68)) == -1 and b"8-byte" in lib.bnerv_last_error()
    for bad in (dict(B=0), dict(B=70000), dict(h=0), dict(w=0)):
        assert sse(**bad) == -1

    for bad in (dict(src=None), dict(out=None)):
        assert luma(**bad) == -1 and b"yuv_luma_f32: null" in lib.bnerv_last_error()
    for bad in (dict(top=3), dict(left=3), dict(h=5), dict(w=6), dict(top=-1), dict(h=0), dict(w=0), dict(top=2 ** 31 - 1)):
        assert luma(**bad) == -1 and b"leaves" in lib.bnerv_last_error(), bad
    assert luma(bps=3) == -1 and b"bytes_per_sample" in lib.bnerv_last_error()
    assert luma(stride=23) == -1 and b"smaller than a frame" in lib.bnerv_last_error()
    assert luma(out=C.c_void_p(66)) == -1 and b"4-byte" in lib.bnerv_last_error()
    assert luma(maxcode=0.0) == -1 and b"maxcode" in lib.bnerv_last_error()
