"""Raw planar YUV 4:2:0 video in and out: the file reader, the float64 restatement of the colour conversion (the
CPU / --host_frames path of the loader and the oracle of the GPU tests), the writer and the per-plane PSNR codecs are scored with.
The device path is csrc/yuv.hip behind ops.yuv420_to_rgb / ops.rgb_to_yuv420; ops.yuv420_sse / ops.yuv_luma_f32 behind codec.Decoder.score
 are the device form of psnr_planes' sums.

A frame is plane Y [H, W], then U [H/2, W/2], then V [H/2, W/2]; frames follow each other without a header.  yuv420p: one byte per
sample; yuv420p10le: two bytes, little endian, values 0..1023."""
import builtins
import os
import re

import numpy as np

PIX_FMTS = {"yuv420p": 8, "yuv420p10le": 10}
MATRICES = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}          # (Kr, Kb); Kg = 1 - Kr - Kb
RANGES = ("limited", "full")


def pix_fmt_of(depth):
    for name, d in PIX_FMTS.items():
        if d == int(depth):
            return name
    raise ValueError(f"yuvio: no 4:2:0 pixel format of {depth} bits here ({', '.join(PIX_FMTS)})")


class Coefficients:
    """What the kernels and the restatement need of a (matrix, range, depth) choice, in float64:
        offset [3], denom [3]   load:  Y' = (Y - offset[0]) / denom[0], Cb' = (U - offset[1]) / denom[1], Cr' likewise
                                store: code = floor(offset[p] + denom[p] * value + 0.5), clamped to [0, maxcode]
        to_rgb [3, 3]           (R, G, B) = to_rgb @ (Y', Cb', Cr')
        to_yuv [3, 3]           (Y', Cb', Cr') = to_yuv @ (R, G, B)
    load_struct() / store_struct() round them to the fp32 struct the kernels take by value."""

    def __init__(self, matrix="bt709", range="limited", depth=8):
        if matrix not in MATRICES:
            raise ValueError(f"yuvio: matrix {matrix!r} (one of {', '.join(MATRICES)})")
        if range not in RANGES:
            raise ValueError(f"yuvio: range {range!r} (one of {', '.join(RANGES)})")
        depth = PIX_FMTS.get(depth, depth)
        if depth not in PIX_FMTS.values():
            raise ValueError(f"yuvio: bit depth {depth!r} (8 or 10)")
        self.matrix, self.range, self.depth = matrix, range, int(depth)
        self.pix_fmt = pix_fmt_of(depth)
        self.bytes_per_sample = 1 if depth == 8 else 2
        self.dtype = np.dtype(np.uint8) if depth == 8 else np.dtype("<u2")
        self.maxcode = 2 ** depth - 1
        s = float(2 ** (depth - 8))
        kr, kb = MATRICES[matrix]
        kg = 1.0 - kr - kb
        if range == "limited":
            self.offset = np.array([16 * s, 128 * s, 128 * s], dtype=np.float64)
            self.denom = np.array([219 * s, 224 * s, 224 * s], dtype=np.float64)
        else:
            self.offset = np.array([0.0, 2.0 ** (depth - 1), 2.0 ** (depth - 1)], dtype=np.float64)
            self.denom = np.full(3, float(self.maxcode), dtype=np.float64)
        self.to_rgb = np.array([[1.0, 0.0, 2 * (1 - kr)],
                                [1.0, -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg],
                                [1.0, 2 * (1 - kb), 0.0]], dtype=np.float64)
        y = np.array([kr, kg, kb], dtype=np.float64)
        self.to_yuv = np.stack([y, (np.array([0.0, 0.0, 1.0]) - y) / (2 * (1 - kb)), (np.array([1.0, 0.0, 0.0]) - y) / (2 * (1 - kr))])

    def _struct(self, m, scale):
        from . import _lib as L
        c = L.YuvCoeffs()
        c.m[:] = [float(v) for v in m.reshape(-1)]
        c.off[:] = [float(v) for v in self.offset]
        c.scale[:] = [float(v) for v in scale]
        c.maxcode = float(self.maxcode)
        return c

    def load_struct(self):
        return self._struct(self.to_rgb, 1.0 / self.denom)

    def store_struct(self):
        return self._struct(self.to_yuv, self.denom)

    def __repr__(self):
        return f"Coefficients({self.matrix!r}, {self.range!r}, {self.depth})"


def coefficients(matrix="bt709", range="limited", depth=8):
    return Coefficients(matrix, range, depth)


def crop_offsets(src_h, src_w, ch, cw):
    """(top, left) of the reference's centre crop (hnerv_utils._center_crop)."""
    if ch > src_h or cw > src_w:
        raise NotImplementedError(f"frames of {src_h}x{src_w} are smaller than the {ch}x{cw} crop (the bicubic up-sampling branch is not supported)")
    return int(round((src_h - ch) / 2.0)), int(round((src_w - cw) / 2.0))


def frame_samples(height, width):
    return height * width * 3 // 2


# ----------------------------------------------------------------------------------------------------------------------
# the float64 restatement of DESIGN section 25
# ----------------------------------------------------------------------------------------------------------------------
def to_rgb_reference(y, u, v, coeffs, crop=None):
    """Planes of sample codes ([..., H, W], [..., H/2, W/2] twice) -> float64 RGB [..., 3, ch, cw] in [0, 1].
    crop = (top, left, ch, cw) in source coordinates (any parity); None: the whole frame."""
    y, u, v = (np.asarray(a) for a in (y, u, v))
    H, W = y.shape[-2:]
    if H % 2 or W % 2 or u.shape[-2:] != (H // 2, W // 2) or v.shape != u.shape:
        raise ValueError(f"yuvio: planes {y.shape}, {u.shape}, {v.shape} are no 4:2:0 frame of even size")
    top, left, ch, cw = (0, 0, H, W) if crop is None else crop
    if not (0 <= top and 0 <= left and ch > 0 and cw > 0 and top + ch <= H and left + cw <= W):
        raise ValueError(f"yuvio: the crop {crop} leaves the {H}x{W} frame")
    H2, W2 = H // 2, W // 2
    yy, xx = np.arange(top, top + ch), np.arange(left, left + cw)
    j = yy >> 1
    n = np.where(yy % 2 == 0, np.maximum(j - 1, 0), np.minimum(j + 1, H2 - 1))
    i = xx >> 1
    i2 = np.where(xx % 2 == 1, np.minimum(i + 1, W2 - 1), i)             # even x: 0.5 (C + C) = C
    planes = [y[..., top:top + ch, left:left + cw].astype(np.float64)]
    for c in (u, v):
        c = c.astype(np.float64)
        cv = 0.75 * c[..., j, :] + 0.25 * c[..., n, :]
        planes.append(0.5 * (cv[..., i] + cv[..., i2]))
    norm = [(p - coeffs.offset[k]) / coeffs.denom[k] for k, p in enumerate(planes)]
    rgb = [coeffs.to_rgb[c, 0] * norm[0] + coeffs.to_rgb[c, 1] * norm[1] + coeffs.to_rgb[c, 2] * norm[2] for c in range(3)]
    return np.clip(np.stack(rgb, axis=-3), 0.0, 1.0)


def to_yuv_reference(rgb, coeffs, return_pre=False):
    """RGB [..., 3, H, W] (any float; clamped to [0, 1]) -> (y, u, v) planes of sample codes in the depth's dtype.
    return_pre=True: also the float64 values offset + scale * value the codes are floor(. + 0.5) of, as a second triple."""
    rgb = np.clip(np.asarray(rgb, dtype=np.float64), 0.0, 1.0)
    H, W = rgb.shape[-2:]
    if rgb.shape[-3] != 3 or H % 2 or W % 2:
        raise ValueError(f"yuvio: {rgb.shape} is no [..., 3, H, W] frame of even size")
    R, G, B = rgb[..., 0, :, :], rgb[..., 1, :, :], rgb[..., 2, :, :]
    m = coeffs.to_yuv
    vals = [m[p, 0] * R + m[p, 1] * G + m[p, 2] * B for p in range(3)]
    xe = np.arange(0, W, 2)
    for p in (1, 2):
        c = vals[p]
        h = (c[..., np.maximum(xe - 1, 0)] + 2.0 * c[..., xe] + c[..., xe + 1]) / 4.0
        vals[p] = 0.5 * (h[..., 0::2, :] + h[..., 1::2, :])
    pre = [coeffs.offset[p] + coeffs.denom[p] * vals[p] for p in range(3)]
    codes = tuple(np.clip(np.floor(a + 0.5), 0, coeffs.maxcode).astype(coeffs.dtype) for a in pre)
    return (codes, tuple(pre)) if return_pre else codes


def parse_weights(text):
    """'6_1_1' (the CLI form) or three numbers -> (w_y, w_u, w_v) floats: none negative, a positive sum."""
    parts = str(text).split("_") if isinstance(text, str) else list(text)
    try:
        w = tuple(float(p) for p in parts)
    except (TypeError, ValueError):
        w = ()
    if len(w) != 3 or min(w) < 0 or not 0 < sum(w) < float("inf"):
        raise ValueError(f"yuvio: plane weights {text!r} are not three numbers Y_U_V, none negative, with a positive sum")
    return w


def plane_loss_reference(rgb, planes, coeffs, window=(0, 0), weights=(6, 1, 1), return_pre=False):
    """The float64 restatement of the plane loss.  rgb [B, 3, H, W], any float, H and W even, NOT clamped;
    planes = (y, u, v) integer codes [B, src_h, src_w], [B, src_h/2, src_w/2] twice: sample b is compared against the H x W window at
    window = (top, left), both even, of frame b.  Returns (L [B], mse [B, 3], grad [B, 3, H, W]): grad is d mean_b(L[b]) / d rgb, written
    out analytically by the adjoint taps.  return_pre=True: also the triple a_p = offset + denom * value the errors are taken of -- for
    rgb in [0, 1] the `pre` of to_yuv_reference(rgb, coeffs, return_pre=True)."""
    P = np.asarray(rgb, dtype=np.float64)
    if P.ndim != 4 or P.shape[1] != 3 or P.shape[2] % 2 or P.shape[3] % 2:
        raise ValueError(f"yuvio: {P.shape} is no [B, 3, H, W] batch of even size")
    B, _, H, W = P.shape
    top, left = (int(v) for v in window)
    y, u, v = (np.asarray(a) for a in planes)
    if top % 2 or left % 2 or top < 0 or left < 0 or y.ndim != 3 or y.shape[0] != B or top + H > y.shape[1] or left + W > y.shape[2]:
        raise ValueError(f"yuvio: the {H}x{W} window at (top {top}, left {left}) of luma planes {y.shape} for {B} samples")
    w = np.asarray(parse_weights(weights), dtype=np.float64)
    w = w / w.sum()
    M, m = coeffs.to_yuv, float(coeffs.maxcode)
    src = [y[:, top:top + H, left:left + W].astype(np.float64)]
    src += [c[:, top // 2:top // 2 + H // 2, left // 2:left // 2 + W // 2].astype(np.float64) for c in (u, v)]
    xe = np.arange(0, W, 2)
    pre, err, mse = [], [], np.zeros((B, 3))
    for p in range(3):
        val = M[p, 0] * P[:, 0] + M[p, 1] * P[:, 1] + M[p, 2] * P[:, 2]
        if p:
            h = (val[..., np.maximum(xe - 1, 0)] + 2.0 * val[..., xe] + val[..., xe + 1]) / 4.0
            val = 0.5 * (h[:, 0::2, :] + h[:, 1::2, :])
        a = coeffs.offset[p] + coeffs.denom[p] * val
        e = (a - src[p]) / m
        pre.append(a)
        err.append(e)
        mse[:, p] = (e * e).mean(axis=(1, 2))
    L = mse @ w
    grad = np.zeros_like(P)
    # luma: every pixel its own error
    gy = 2.0 * w[0] * coeffs.denom[0] / (B * m * H * W) * err[0]
    for c in range(3):
        grad[:, c] += M[0, c] * gy
    # chroma: sample (j, i) reaches rows 2j, 2j + 1 (1/2 each) and columns 2i - 1 (1/4; clamped: column 0 takes it twice), 2i (1/2), 2i + 1 (1/4)
    for p in (1, 2):
        ge = 2.0 * w[p] * coeffs.denom[p] / (B * m * (H * W / 4.0)) * 0.5 * err[p]          # [B, H/2, W/2]
        t = np.zeros((B, H // 2, W))
        t[..., xe] += 0.5 * ge
        t[..., xe + 1] += 0.25 * ge
        np.add.at(t, (slice(None), slice(None), np.maximum(xe - 1, 0)), 0.25 * ge)
        t = np.repeat(t, 2, axis=1)
        for c in range(3):
            grad[:, c] += M[p, c] * t
    return (L, mse, grad, tuple(pre)) if return_pre else (L, mse, grad)


def plane_loss_up_reference(rgb, planes, coeffs, size, window=(0, 0), weights=(6, 1, 1)):
    """The float64 restatement of the plane loss through the up-sampler.  rgb [B, 3, h, w], any float, any h and w, NOT
    clamped; size = (H, W), both even: the window at window = (top, left) of the planes that Q = U rgb is compared against, U the two-pass
    table filter of resize.py without its clamp.  The dense Wr [W, w], Wc [H, h] are built from the fp32 words of resize.axis_table -- the
    words the kernels read -- and widened: Q[c] = Wc P[c] Wr^T, (L, mse, gQ) = plane_loss_reference(Q, ...), grad = Wc^T gQ Wr.
    Returns (L [B], mse [B, 3], grad [B, 3, h, w])."""
    from . import resize as R
    P = np.asarray(rgb, dtype=np.float64)
    if P.ndim != 4 or P.shape[1] != 3 or P.size == 0:
        raise ValueError(f"yuvio: {P.shape} is no non-empty [B, 3, h, w] batch")
    H, W = (int(v) for v in size)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"yuvio: 4:2:0 needs even dimensions, size is {H}x{W}")
    h, w = P.shape[2:]
    Wr = R.dense_matrix(*R.axis_table(w, W), w)
    Wc = R.dense_matrix(*R.axis_table(h, H), h)
    Q = Wc @ P @ Wr.T
    L, mse, gQ = plane_loss_reference(Q, planes, coeffs, window, weights)
    return L, mse, Wc.T @ gQ @ Wr


def luma_pre_reference(rgb, planes, coeffs, window=(0, 0), return_pre=False):
    """The float64 restatement of the two planes the MS-SSIM-Y term compares.  rgb [B, 3, H, W], any float, NOT clamped;
    planes = (y, u, v) integer codes as plane_loss_reference takes them (only y [B, src_h, src_w] is read); window = (top, left), any parity.
    Returns (Yp [B, 1, H, W], Ys [B, 1, H, W], k [3]): Yp = (offset_0 + denom_0 (to_yuv[0] . rgb)) / maxcode, the luma code before rounding
    over the peak (for rgb in [0, 1], maxcode * Yp is the luma `pre` of to_yuv_reference); Ys = code / maxcode; k_c = denom_0 to_yuv[0, c] /
    maxcode = d Yp / d rgb[c].  return_pre=True: also a_0 = offset_0 + denom_0 (to_yuv[0] . rgb), the value Yp is the quotient of (the
    division rounds once, so maxcode * Yp itself is a_0 only to an ulp)."""
    P = np.asarray(rgb, dtype=np.float64)
    if P.ndim != 4 or P.shape[1] != 3:
        raise ValueError(f"yuvio: {P.shape} is no [B, 3, H, W] batch")
    B, _, H, W = P.shape
    top, left = (int(v) for v in window)
    y = np.asarray(planes[0] if isinstance(planes, (tuple, list)) else planes)
    if top < 0 or left < 0 or y.ndim != 3 or y.shape[0] != B or top + H > y.shape[1] or left + W > y.shape[2]:
        raise ValueError(f"yuvio: the {H}x{W} window at (top {top}, left {left}) of luma planes {y.shape} for {B} samples")
    M, m = coeffs.to_yuv, float(coeffs.maxcode)
    val = M[0, 0] * P[:, 0] + M[0, 1] * P[:, 1] + M[0, 2] * P[:, 2]
    pre = coeffs.offset[0] + coeffs.denom[0] * val
    Yp = pre / m
    Ys = y[:, top:top + H, left:left + W].astype(np.float64) / m
    k = coeffs.denom[0] * M[0] / m
    return (Yp[:, None], Ys[:, None], k, pre[:, None]) if return_pre else (Yp[:, None], Ys[:, None], k)


# ----------------------------------------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------------------------------------
def parse_name(path):
    """(width, height, pix_fmt) as far as a UVG-style file name tells them (Beauty_1920x1080_120fps_420_8bit_YUV.yuv); None where it does not."""
    name = os.path.basename(str(path))
    size = re.search(r"_(\d+)x(\d+)_", name)
    depth = re.search(r"(?<!\d)(8|10)bit", name)
    return (int(size.group(1)) if size else None, int(size.group(2)) if size else None,
            pix_fmt_of(int(depth.group(1))) if depth else None)


def parse_size(text):
    m = re.fullmatch(r"(\d+)x(\d+)", str(text))
    if not m:
        raise ValueError(f"yuvio: size {text!r} is not WIDTHxHEIGHT")
    return int(m.group(1)), int(m.group(2))


class YuvFile:
    """A raw 4:2:0 clip, memory-mapped.  Size and depth come from the arguments or, where they are None, from a UVG-style file name.

        clip = YuvFile("Beauty_1920x1080_120fps_420_8bit_YUV.yuv")
        len(clip), clip.height, clip.width, clip.pix_fmt
        y, u, v = clip.planes(i)                     numpy views of the mapping
        clip.to_device("cuda", crop=(1080, 1920))    [N, 3, ch, cw] fp32 clip, converted on the device"""

    def __init__(self, path, width=None, height=None, pix_fmt=None):
        nw, nh, nf = parse_name(path)
        width, height, pix_fmt = width or nw, height or nh, pix_fmt or nf
        if not width or not height:
            raise ValueError(f"{path}: the file name carries no _WIDTHxHEIGHT_: set the size (--yuv_size WxH; YuvFile(width=, height=))")
        if pix_fmt is None:
            raise ValueError(f"{path}: the file name carries neither 8bit nor 10bit: set the pixel format (--yuv_fmt yuv420p|yuv420p10le; YuvFile(pix_fmt=))")
        if pix_fmt not in PIX_FMTS:
            raise ValueError(f"{path}: pixel format {pix_fmt!r} (one of {', '.join(PIX_FMTS)})")
        if width % 2 or height % 2:
            raise ValueError(f"{path}: 4:2:0 needs even dimensions, got {width}x{height}")
        self.path, self.width, self.height, self.pix_fmt = str(path), int(width), int(height), pix_fmt
        self.depth = PIX_FMTS[pix_fmt]
        self.bytes_per_sample = 1 if self.depth == 8 else 2
        self.dtype = np.dtype(np.uint8) if self.depth == 8 else np.dtype("<u2")
        self.frame_bytes = frame_samples(self.height, self.width) * self.bytes_per_sample
        size = os.path.getsize(self.path)
        if size == 0 or size % self.frame_bytes:
            raise ValueError(f"{path}: {size} bytes is no whole number of {self.width}x{self.height} {pix_fmt} frames of {self.frame_bytes} bytes "
                             "(wrong --yuv_size / --yuv_fmt, or a truncated file)")
        self.n_frames = size // self.frame_bytes
        self._map = np.memmap(self.path, dtype=np.uint8, mode="r")

    def __len__(self):
        return self.n_frames

    def raw(self, i0, i1):
        """Frames i0 .. i1 as they lie in the file: a uint8 view."""
        return self._map[i0 * self.frame_bytes:i1 * self.frame_bytes]

    def planes(self, i):
        if not 0 <= i < self.n_frames:
            raise IndexError(f"frame {i} of a {self.n_frames}-frame clip")
        s = self.raw(i, i + 1).view(self.dtype)
        hw, q = self.height * self.width, (self.height // 2) * (self.width // 2)
        return (s[:hw].reshape(self.height, self.width), s[hw:hw + q].reshape(self.height // 2, self.width // 2),
                s[hw + q:].reshape(self.height // 2, self.width // 2))

    def crop_window(self, crop):
        ch, cw = (self.height, self.width) if crop is None else crop
        top, left = crop_offsets(self.height, self.width, ch, cw)
        return top, left, int(ch), int(cw)

    def frame_rgb(self, i, crop=None, matrix="bt709", range="limited"):
        """Frame i as fp32 [3, ch, cw] through the float64 restatement (the host path)."""
        return to_rgb_reference(*self.planes(i), coefficients(matrix, range, self.depth), self.crop_window(crop)).astype(np.float32)

    def to_device(self, device, chunk=32, crop=None, matrix="bt709", range="limited", count=None, resize=None):
        """The first `count` (default: all) frames as a resident [N, 3, ch, cw] fp32 clip.  Chunks of frames go through two pinned buffers --
        the host fills one while the copy engine drains the other -- and every chunk is converted with ONE kernel launch.
        resize=(h, w): the clip is [N, 3, h, w]; every chunk is converted into a chunk-sized fp32 scratch and resampled from there into its
        slice of the clip (ops.resize_bicubic): the full-size fp32 clip never exists on the device."""
        import torch
        from . import ops
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("YuvFile.to_device: the conversion kernels need a ROCm GPU (frame_rgb() is the host path)")
        n = self.n_frames if count is None else int(count)
        if not 0 < n <= self.n_frames:
            raise ValueError(f"YuvFile.to_device: count={count} of a {self.n_frames}-frame clip")
        top, left, ch, cw = self.crop_window(crop)
        coeffs = coefficients(matrix, range, self.depth)
        chunk = max(1, min(int(chunk), n))
        if resize is None:
            clip = torch.empty(n, 3, ch, cw, dtype=torch.float32, device=device)
        else:
            rh, rw = (int(v) for v in resize)
            clip = torch.empty(n, 3, rh, rw, dtype=torch.float32, device=device)
            full = torch.empty(chunk, 3, ch, cw, dtype=torch.float32, device=device)
            scratch = torch.empty(chunk * 3 * ch * rw, dtype=torch.float32, device=device)
        pinned = [torch.empty(chunk * self.frame_bytes, dtype=torch.uint8, pin_memory=True) for _ in (0, 1)]
        staged = [torch.empty(chunk * self.frame_bytes, dtype=torch.uint8, device=device) for _ in (0, 1)]
        events = [torch.cuda.Event() for _ in (0, 1)]
        with torch.cuda.device(device):
            for k, i0 in enumerate(builtins.range(0, n, chunk)):      # (`range` is a parameter here)
                i1, slot = min(i0 + chunk, n), k % 2
                nbytes = (i1 - i0) * self.frame_bytes
                if k >= 2:
                    events[slot].synchronize()                       # the copy that last read this pinned buffer is done
                pinned[slot].numpy()[:nbytes] = self.raw(i0, i1)
                staged[slot][:nbytes].copy_(pinned[slot][:nbytes], non_blocking=True)
                events[slot].record()
                if resize is None:
                    ops.yuv420_to_rgb(staged[slot], coeffs, i1 - i0, self.height, self.width, crop=(top, left, ch, cw), out=clip[i0:i1])
                else:
                    ops.yuv420_to_rgb(staged[slot], coeffs, i1 - i0, self.height, self.width, crop=(top, left, ch, cw), out=full[:i1 - i0])
                    ops.resize_bicubic(full[:i1 - i0], (rh, rw), out=clip[i0:i1], scratch=scratch)
            torch.cuda.current_stream().synchronize()
        return clip

    def raw_to_device(self, device, count=None, chunk=32):
        """The first `count` (default: all) frames as they lie in the file, one uint8 [n * frame_bytes] device tensor: what the plane loss
        (ops.yuv420_loss) compares against.  1.5 (8 bit) or 3 (10 bit) bytes per pixel and frame beside the 12 of the
        fp32 clip.  The same two pinned buffers as to_device: the host fills one while the copy engine drains the other."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("YuvFile.raw_to_device: the resident raw clip lives on a ROCm GPU (raw() is the host view)")
        n = self.n_frames if count is None else int(count)
        if not 0 < n <= self.n_frames:
            raise ValueError(f"YuvFile.raw_to_device: count={count} of a {self.n_frames}-frame clip")
        chunk = max(1, min(int(chunk), n))
        out = torch.empty(n * self.frame_bytes, dtype=torch.uint8, device=device)
        pinned = [torch.empty(chunk * self.frame_bytes, dtype=torch.uint8, pin_memory=True) for _ in (0, 1)]
        events = [torch.cuda.Event() for _ in (0, 1)]
        with torch.cuda.device(device):
            for k, i0 in enumerate(builtins.range(0, n, chunk)):
                i1, slot = min(i0 + chunk, n), k % 2
                nbytes = (i1 - i0) * self.frame_bytes
                if k >= 2:
                    events[slot].synchronize()                       # the copy that last read this pinned buffer is done
                pinned[slot].numpy()[:nbytes] = self.raw(i0, i1)
                out[i0 * self.frame_bytes:i1 * self.frame_bytes].copy_(pinned[slot][:nbytes], non_blocking=True)
                events[slot].record()
            torch.cuda.current_stream().synchronize()
        return out


def write(path, frames, pix_fmt="yuv420p", append=False):
    """Write frames to a raw file.  frames: an iterable of (y, u, v) plane triples or of 1-D arrays of 1.5 H W samples in file layout
    (what Decoder.frames_yuv yields).  Returns the number of frames written."""
    dtype = np.dtype(np.uint8) if PIX_FMTS[pix_fmt] == 8 else np.dtype("<u2")
    n = 0
    with open(path, "ab" if append else "wb") as f:
        for frame in frames:
            for part in (frame if isinstance(frame, (tuple, list)) else (frame,)):
                a = np.asarray(part)
                if a.dtype.kind not in "ui" or a.min(initial=0) < 0 or a.max(initial=0) > 2 ** PIX_FMTS[pix_fmt] - 1:
                    raise ValueError(f"yuvio.write: samples must be integer codes in 0..{2 ** PIX_FMTS[pix_fmt] - 1}")
                np.ascontiguousarray(a.astype(dtype, copy=False)).tofile(f)
            n += 1
    return n


def psnr_from_sse(sse_yuv, n_luma, depth):
    """The formula part of psnr_planes: (SSE-Y, SSE-U, SSE-V) of one 4:2:0 frame of n_luma luma samples (each chroma plane has n_luma / 4;
    a triple gives the three sample counts themselves) -> {"psnr_y", "psnr_u", "psnr_v", "psnr_yuv"}: 10 log10(peak^2 n / SSE) with
    peak = 2^depth - 1 (inf at SSE 0) and (6 Y + U + V) / 8.  The sums are taken as exact Python integers, so a sum from the device
    (ops.yuv420_sse) gives the floats psnr_planes gives."""
    peak = 2 ** int(depth) - 1
    sizes = tuple(int(n) for n in n_luma) if isinstance(n_luma, (tuple, list)) else (int(n_luma), int(n_luma) // 4, int(n_luma) // 4)
    out = {}
    for name, sse, n in zip("yuv", sse_yuv, sizes):
        sse = int(sse)
        out[f"psnr_{name}"] = float("inf") if sse == 0 else 10.0 * float(np.log10(peak * peak * n / sse))
    out["psnr_yuv"] = (6.0 * out["psnr_y"] + out["psnr_u"] + out["psnr_v"]) / 8.0
    return out


def psnr_planes(a, b, depth):
    """Per-plane distortion of two frames given as (y, u, v) triples of integer codes: the sums of squared errors as exact Python integers,
    PSNR-Y / -U / -V = 10 log10(peak^2 n / SSE) with peak = 2^depth - 1 (inf at SSE 0), and PSNR-YUV = (6 Y + U + V) / 8."""
    sse, sizes = [], []
    for name, pa, pb in zip("yuv", a, b):
        pa, pb = np.asarray(pa), np.asarray(pb)
        if pa.shape != pb.shape:
            raise ValueError(f"psnr_planes: plane {name}: {pa.shape} against {pb.shape}")
        d = pa.astype(np.int64) - pb.astype(np.int64)
        sse.append(int((d * d).sum()))
        sizes.append(pa.size)
    psnr = psnr_from_sse(sse, sizes, depth)
    out = {}
    for name, s in zip("yuv", sse):
        out[f"sse_{name}"], out[f"psnr_{name}"] = s, psnr[f"psnr_{name}"]
    out["psnr_yuv"] = psnr["psnr_yuv"]
    return out
