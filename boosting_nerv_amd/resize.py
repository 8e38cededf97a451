"""The loader's frame resize (--resize_list H_W), host side: the definition the kernels of csrc/resize.hip are tested
against and the --host_frames path of the loader.

The filter is the separable antialiased bicubic of torch.nn.functional.interpolate(mode='bicubic', align_corners=False, antialias=True):
the Keys cubic with a = -0.5, stretched by s = max(scale, 1) where scale = n_in / n_out.  Output index i of an axis sits at
c = scale * (i + 0.5) and reads the inputs

    first = max(0, int(c - 2 s + 0.5))   ..   end - 1,  end = min(int(c + 2 s + 0.5), n_in)
    w_j   = cubic((j - c + 0.5) / s),  divided by the sum over the taps

Weights are formed and normalised in float64 and rounded to fp32 once.  At equal size every output has the single non-zero weight 1.0 on
its own input: the resize returns its input exactly.

    axis_table(n_in, n_out)            (first int32 [n_out], count int32 [n_out], weights fp32 [n_out, T]), rows zero-padded to T = max(count)
    resize_reference(x, (h, w))        the fp32 definition: horizontal pass, then vertical, acc = fp32(acc + fp32(w_j * x_j)) over the taps
                                       in ascending j from 0.0f, an fp32 intermediate, a final clamp to [0, 1]; ops.resize_bicubic gives its bits
    resize_reference64(x, (h, w))      the same with float64 tables and sums (for error bounds)
    adjoint_table(n_in, n_out)         the transpose of axis_table in the same shape, per INPUT sample (the gradient
                                       of a loss taken through the resize)
    parse_resize('-1' | 'H_W')         None | (H, W)

An axis whose outputs need more than MAX_TAPS = 64 taps (a reduction of more than about 15x) is refused with a ValueError."""
import re

import numpy as np

MAX_TAPS = 64      # BNERV_RESIZE_MAX_TAPS
STRIP = 64         # BNERV_RESIZE_STRIP: output columns of a block of the row pass
_A = -0.5


def cubic(x):
    """The Keys cubic convolution kernel (a = -0.5), float64, elementwise."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((_A + 2.0) * x - (_A + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * _A
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _axis_table64(n_in, n_out):
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize: an axis of {n_in} -> {n_out} samples")
    scale = n_in / n_out
    s = max(scale, 1.0)
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    first = np.maximum(0, (c - 2.0 * s + 0.5).astype(np.int64))            # (astype truncates towards zero, like int())
    end = np.minimum((c + 2.0 * s + 0.5).astype(np.int64), n_in)
    count = end - first
    T = int(count.max())
    if T > MAX_TAPS:
        raise ValueError(f"resize: {n_in} -> {n_out} samples needs {T} taps per output, the limit is {MAX_TAPS} (a reduction of about 15x)")
    tap = np.arange(T, dtype=np.int64)[None, :]
    w = cubic((first[:, None] + tap - c[:, None] + 0.5) / s)
    w[tap >= count[:, None]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    return first.astype(np.int32), count.astype(np.int32), w


_tables = {}


def axis_table(n_in, n_out):
    """(first int32 [n_out], count int32 [n_out], weights fp32 [n_out, T]) of one axis; cached by (n_in, n_out), read-only arrays."""
    key = (int(n_in), int(n_out))
    if key not in _tables:
        first, count, w = _axis_table64(*key)
        got = (first, count, w.astype(np.float32))
        for a in got:
            a.setflags(write=False)
        _tables[key] = got
    return _tables[key]


_adjoints = {}


def adjoint_table(n_in, n_out):
    """The transpose of axis_table(n_in, n_out) in the same table shape, so pack_table packs it and strip_span sizes its
    LDS pitch: (first int32 [n_in], count int32 [n_in], weights fp32 [n_in, Ta]).  Input i lists the contiguous range of outputs whose tap
    range holds i -- contiguous because first and first + count do not decrease along the axis -- and entry k is the forward table's fp32
    word w[first_out + k][i - first[first_out + k]].  An input no output reads gets count 0 (a zero gradient).  Ta > MAX_TAPS (an
    enlargement of more than about 16x): ValueError.  Cached by (n_in, n_out), read-only arrays."""
    key = (int(n_in), int(n_out))
    if key not in _adjoints:
        first, count, w = axis_table(*key)
        f64, e64 = first.astype(np.int64), first.astype(np.int64) + count.astype(np.int64)
        if np.any(np.diff(f64) < 0) or np.any(np.diff(e64) < 0):
            raise ValueError(f"resize: the tap ranges of {key[0]} -> {key[1]} samples are not monotone")
        i = np.arange(key[0], dtype=np.int64)
        lo = np.searchsorted(e64, i, side="right")                     # outputs with end <= i: those in front of the range
        hi = np.searchsorted(f64, i, side="right")                     # outputs with first <= i
        cnt = np.maximum(hi - lo, 0)
        Ta = max(int(cnt.max()), 1)
        if Ta > MAX_TAPS:
            raise ValueError(f"resize: the adjoint of {key[0]} -> {key[1]} samples needs {Ta} taps per input, the limit is {MAX_TAPS} "
                             "(an enlargement of about 16x)")
        wa = np.zeros((key[0], Ta), dtype=np.float32)
        k = np.arange(Ta, dtype=np.int64)[None, :]
        o = np.minimum(lo[:, None] + k, key[1] - 1)
        live = k < cnt[:, None]
        j = np.clip(i[:, None] - f64[o], 0, w.shape[1] - 1)
        wa[live] = w[o, j][live]
        got = (lo.astype(np.int32), cnt.astype(np.int32), wa)
        for a in got:
            a.setflags(write=False)
        _adjoints[key] = got
    return _adjoints[key]


def dense_matrix(first, count, weights, n_cols):
    """The dense float64 matrix [len(first), n_cols] of a table: row r holds weights[r, :count[r]] at columns first[r] ..; the fp32 words, widened."""
    m = np.zeros((len(first), int(n_cols)), dtype=np.float64)
    for r in range(len(first)):
        m[r, first[r]:first[r] + count[r]] = weights[r, :count[r]]
    return m


def strip_span(first, count, strip=STRIP):
    """The LDS pitch of the row pass, in floats: the widest input span of `strip` consecutive outputs, measured from the strip's first input
    rounded down to a multiple of 4 (the 16-byte staging starts there), rounded up to a multiple of 4."""
    first, end = np.asarray(first, dtype=np.int64), np.asarray(first, dtype=np.int64) + np.asarray(count, dtype=np.int64)
    lo = first[::strip] & ~3
    hi = np.array([end[o:o + strip].max() for o in range(0, first.size, strip)], dtype=np.int64)
    return int(-(-int((hi - lo).max()) // 4) * 4)


def pack_table(first, count, weights):
    """The device form of an axis table (include/bnerv.h): int32 first | int32 count | fp32 weights [n_out, T] | fp32 weights [T, n_out], as
    one int32 array of (2 + 2 T) n_out words."""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    return np.concatenate([np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32), w.reshape(-1).view(np.int32),
                           np.ascontiguousarray(w.T).reshape(-1).view(np.int32)])


def _apply(x, first, count, weights, axis):
    """One pass along `axis` (-1 or -2) in the dtype of `weights`: the sum over the taps in ascending order, every product and every sum
    rounded on its own (numpy never fuses them).  A padded tap adds nothing."""
    dt = weights.dtype
    n_in, T = x.shape[axis], weights.shape[1]
    idx = np.minimum(first.astype(np.int64)[:, None] + np.arange(T)[None, :], n_in - 1)
    shape = list(x.shape)
    shape[axis] = first.size
    acc = np.zeros(shape, dtype=dt)
    for j in range(T):
        live = j < count
        if axis == -1:
            p = weights[:, j] * x[..., idx[:, j]]
            acc = acc + np.where(live, p, dt.type(0))
        else:
            p = weights[:, j][:, None] * x[..., idx[:, j], :]
            acc = acc + np.where(live[:, None], p, dt.type(0))
    return acc


def _resize(x, size, clamp, dt):
    import torch
    as_torch = torch.is_tensor(x)
    a = x.detach().cpu().numpy() if as_torch else np.asarray(x)
    if a.ndim < 2 or a.size == 0:
        raise ValueError(f"resize: need a non-empty [..., H, W] array, got {a.shape}")
    a = np.ascontiguousarray(a, dtype=dt)
    h, w = (int(v) for v in size)
    tables = []
    for n_in, n_out in ((a.shape[-1], w), (a.shape[-2], h)):
        if dt == np.float32:
            tables.append(axis_table(n_in, n_out))
        else:
            tables.append(_axis_table64(n_in, n_out))
    out = _apply(_apply(a, *tables[0], -1), *tables[1], -2)
    if clamp:
        out = np.clip(out, dt(0), dt(1))
    return torch.from_numpy(out) if as_torch else out


def resize_reference(x, size, clamp=True):
    """x [..., H, W] (numpy array or torch tensor; computed in fp32) -> [..., h, w] fp32 of the same kind: the definition."""
    return _resize(x, size, clamp, np.float32)


def resize_reference64(x, size, clamp=True):
    """resize_reference with float64 tables (not rounded to fp32), products and sums."""
    return _resize(x, size, clamp, np.float64)


def parse_resize(text):
    """'-1' -> None (no resize); 'H_W' -> (H, W), both positive.  Anything else: ValueError."""
    text = str(text).strip()
    if text == "-1":
        return None
    m = re.fullmatch(r"(\d+)_(\d+)", text)
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"--resize_list {text!r}: -1 (no resize) or H_W with H, W >= 1")
    return int(m.group(1)), int(m.group(2))


def describe(src_hw, dst_hw):
    """The run log's line."""
    th, tw = axis_table(src_hw[0], dst_hw[0])[2].shape[1], axis_table(src_hw[1], dst_hw[1])[2].shape[1]
    return f"Resize: {src_hw[0]}x{src_hw[1]} -> {dst_hw[0]}x{dst_hw[1]} (antialiased bicubic), {th} x {tw} taps"
