"""The descriptor table of tests/test_conv_route_cpu.py: conv, weight-gradient and pair descriptors with made-up pointers (as
tests/test_alignment_cpu.py: the host queries never dereference them) that straddle every threshold of the kernel selection in
csrc/ (route.h).  tools/record_conv_route.py asks a build of the library for its answers to the three long-standing queries over this
table and writes tests/conv_route_answers.json; the table is deterministic, rows are identified by their index."""
import ctypes as C

from boosting_nerv_amd import _lib as L

BASE = 0x7F0000000000        # a made-up, 16-byte aligned "device" address
CH = (8, 9, 12, 13, 16, 17, 32, 33, 64, 65, 96, 97, 127, 128)
PTRS = ("x", "w", "bias", "out", "out2", "aux0", "aux1", "aux2", "scale", "shift", "partial")
INS = (L.IN_PLAIN, L.IN_AFFINE, L.IN_GELU_AFFINE, L.IN_UNSHUFFLE, L.IN_TANHGRAD)
EPS = (L.EP_BIAS, L.EP_BIAS_SIN, L.EP_BIAS_RES, L.EP_BIAS_TANH, L.EP_PLAIN, L.EP_DGELU, L.EP_DSIN, L.EP_BIAS_GELU, L.EP_DGELU_SAVED)
SUMS = (L.EP_DGELU, L.EP_DSIN, L.EP_DGELU_SAVED)


def _p(i, off=0):
    return BASE + 0x1000000 * i + off


def conv_row(Cin, Cout, H, W, *, k=3, B=1, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS, in_s=1, out_s=1, transposed=0, partial=False, off=None,
             env=None, ctx=True):
    """One row: the integer fields, which optional pointers are set, byte offsets of pointers, and environment switches."""
    return dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=in_mode, ep_mode=ep_mode, in_s=in_s, out_s=out_s, transposed=transposed,
                partial=partial, off=dict(off or {}), env=dict(env or {}), ctx=ctx)


def conv_desc(r, partial=None):
    """The ConvDesc of a row; every tensor the modes could read is present.  partial: override the row's choice (True / False)."""
    off = r["off"]
    ptr = {n: C.c_void_p(_p(i, off.get(n, 0))) for i, n in enumerate(PTRS)}
    if not (r["partial"] if partial is None else partial):
        ptr["partial"] = None
    wCo, wCi = (r["Cin"], r["Cout"]) if r["transposed"] else (r["Cout"], r["Cin"])
    return L.ConvDesc(*[ptr[n] for n in PTRS], r["B"], r["Cin"], r["Cout"], r["H"], r["W"], r["k"], r["in_mode"], r["ep_mode"], r["in_s"],
                      r["out_s"], r["transposed"], wCo, wCi, C.c_void_p(_p(15)) if r["ctx"] else None)


def conv_rows():
    rows = []
    add = lambda *a, **kw: rows.append(conv_row(*a, **kw))
    tall = lambda px: [(px // 4 - 1, 4), (px // 4, 4), (px // 4 + 1, 4)]         # pixel counts px - 4, px, px + 4 with float4 rows
    # channel thresholds, both sides: forward, TAT forward and its data gradient, low resolution and 180x320
    for ci in CH:
        for co in CH:
            add(ci, co, 32, 32)
    for c in CH:
        add(c, c, 32, 32, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_GELU)
        add(c, c, 32, 32, ep_mode=L.EP_DGELU_SAVED, transposed=1)
        add(c, c, 180, 320, ep_mode=L.EP_DSIN, transposed=1)
        add(c, c, 180, 320, in_mode=L.IN_GELU_AFFINE, ep_mode=L.EP_BIAS_RES)
        add(c, 4 * c, 90, 160, ep_mode=L.EP_BIAS_SIN, out_s=2)
        add(4 * c, c, 90, 160, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=2, transposed=1)
        add(c, c, 32, 32, k=1)
    # pixel-count thresholds
    for px in (256, 1024, 4096, 16384, 65536):
        side = int(px ** 0.5)
        for H, W in tall(px) + [(side, side)]:
            add(30, 30, H, W, ep_mode=L.EP_DGELU_SAVED, transposed=1)
            add(12, 48, H, W, ep_mode=L.EP_BIAS_SIN, out_s=2)
            add(48, 12, H, W, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=2, transposed=1)
            add(95, 95, H, W, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_RES)
            add(95, 95, H, W, ep_mode=L.EP_DSIN, transposed=1)
            add(38, 3, H, W, ep_mode=L.EP_BIAS_TANH)                             # the 3x3 head
            add(12, 3, H, W, k=1, ep_mode=L.EP_BIAS_TANH)                        # the 1x1 head and its data gradient
            add(3, 12, H, W, k=1, in_mode=L.IN_TANHGRAD, ep_mode=L.EP_PLAIN, transposed=1)
            for part in (False, True):                                           # long K: split-K, and the stem kernel up to 256 pixels
                add(750, 30, H, W, ep_mode=L.EP_PLAIN, transposed=1, partial=part)
                add(1975, 95, H, W, in_mode=L.IN_UNSHUFFLE, in_s=5, ep_mode=L.EP_PLAIN, transposed=1, partial=part)
                add(128, 96, H, W, ep_mode=L.EP_PLAIN, transposed=1, partial=part)
                add(127, 97, H, W, ep_mode=L.EP_PLAIN, transposed=1, partial=part)
    add(3, 38, 128, 256, ep_mode=L.EP_PLAIN, transposed=1)                       # the 3x3 head's data gradient (above the low-resolution family's images)
    add(3, 38, 128, 256, in_mode=L.IN_TANHGRAD, ep_mode=L.EP_PLAIN, transposed=1)
    add(3, 38, 128, 256, ep_mode=L.EP_PLAIN, transposed=1, partial=True)
    # the 16-tile bound of the wide split kernels (8x32 tiles x batch), with the default and a lowered bound
    for H, W, B in ((32, 96, 1), (32, 128, 1), (36, 132, 1), (24, 128, 1), (40, 96, 1), (8, 32, 15), (8, 32, 16), (8, 32, 17)):
        for env in ({}, {"BNERV_SPLIT_WIDE_MIN_TILES": "1"}, {"BNERV_SMALL": "0"}, {"BNERV_SMALL": "0", "BNERV_SPLIT_WIDE_MIN_TILES": "13"}):
            add(30, 30, H, W, B=B, ep_mode=L.EP_DSIN, transposed=1, env=env)
            add(64, 64, H, W, B=B, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_GELU, env=env)
            add(30, 30, H, W, B=B, ep_mode=L.EP_DSIN, transposed=1, env=env, ctx=False)
    # rows that are not float4-aligned, and each operand 4 bytes off
    for ci, co, H, W in ((12, 12, 48, 96), (30, 30, 9, 16), (30, 30, 36, 132), (64, 64, 64, 128), (95, 95, 9, 16)):
        for ep in (L.EP_DGELU_SAVED, L.EP_DSIN, L.EP_DGELU, L.EP_PLAIN):
            add(ci, co, H, W - 1, ep_mode=ep, transposed=1)
            add(ci, co, H, W - 2, ep_mode=ep, transposed=1)
            for name in ("x", "out", "out2", "aux0", "aux1", "aux2", "partial", "w", "scale"):
                add(ci, co, H, W, ep_mode=ep, transposed=1, off={name: 4}, partial=(name == "partial"))
    # shuffle factors
    for s in (1, 2, 3, 5):
        for c in (12, 15, 30):
            for H, W in ((9, 16), (45, 80), (90, 160), (180, 320)):
                add(c, c * s * s, H, W, ep_mode=L.EP_BIAS_SIN, out_s=s)
                add(c, c * s * s, H, W, ep_mode=L.EP_BIAS, out_s=s)
                add(c * s * s, c, H, W, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=s, transposed=1)
                add(c * s * s, c, H, W, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=s, transposed=1, partial=True)
    # every (in, ep) pair, on a layer of each family's kind
    for i in INS:
        for e in EPS:
            for ci, co, H, W, env in ((12, 12, 64, 64, {}), (30, 30, 32, 32, {}), (30, 30, 64, 128, {}), (64, 64, 32, 32, {"BNERV_SMALL": "0"}),
                                      (95, 95, 9, 16, {}), (16, 16, 64, 64, {})):
                add(ci, co, H, W, in_mode=i, ep_mode=e, env=env)
                add(ci, co, H, W, k=1, in_mode=i, ep_mode=e, env=env)
    return rows


def changed_rows():
    """The rows on which bnerv_conv_partial_rows answers otherwise than the commit before the routes did, ON PURPOSE:
    a 3 -> C data gradient with EP_PLAIN and no workspace on 4096..16384 pixels.  The launch runs the 3x3 head kernel (8x32 grid, no rows
    written); the old query named the 4x16 tiles of the low-resolution family, which takes the layer only when a workspace is passed.
    Kept out of conv_rows(), whose answers must be equal; the recorded file holds the old answers under "conv_changed"."""
    return [conv_row(3, 38, H, W, ep_mode=L.EP_PLAIN, transposed=1) for H, W in ((64, 64), (64, 128), (1024, 4), (4096, 4))]       # both ends of that range


def wgrad_dims():
    """(B, Cin, Cout, H, W, k) of bnerv_conv_wgrad_ws_bytes."""
    dims = []
    for k in (1, 3):
        for ci in CH:
            for co in CH:
                dims.append((1, ci, co, 32, 32, k))
        for c in CH + (3, 38, 48, 95, 750):
            for H, W in ((9, 16), (16, 16), (13, 20), (36, 64), (64, 64), (72, 128), (32, 96), (32, 128), (36, 132), (180, 320), (720, 1280)):
                for B in (1, 2, 16):
                    dims.append((B, c, c, H, W, k))
                dims.append((1, c, 4 * c, H, W, k))
                dims.append((1, 12, c, H, W, k))
    return dims


def wgrad_desc(B, Cin, Cout, H, W, k, *, in_mode=L.IN_PLAIN, g_mode=L.IN_PLAIN, g_s=1, off=None, ws_bytes=0, defer=1, x=None, g=None):
    off = off or {}
    return L.WgradDesc(C.c_void_p(x or _p(16, off.get("x", 0))), C.c_void_p(g or _p(17, off.get("g", 0))), C.c_void_p(_p(18, off.get("gaux", 0))),
                       C.c_void_p(_p(19)), C.c_void_p(_p(20)), C.c_void_p(_p(21)), C.c_void_p(_p(22)), C.c_void_p(_p(23)), ws_bytes,
                       B, Cin, Cout, H, W, k, in_mode, g_mode, g_s, defer, C.c_void_p(_p(15)))


def wgrad_modes(k):
    """(in_mode, g_mode, g_s, pointer offsets) of the weight-gradient descriptors asked per dimension tuple."""
    m = [(L.IN_PLAIN, L.IN_PLAIN, 1, {}), (L.IN_PLAIN, L.IN_TANHGRAD, 1, {}), (L.IN_PLAIN, L.IN_PLAIN, 1, {"x": 4}), (L.IN_PLAIN, L.IN_PLAIN, 1, {"g": 4}),
         (L.IN_PLAIN, L.IN_TANHGRAD, 1, {"gaux": 4})]
    if k == 3:
        m += [(L.IN_AFFINE, L.IN_PLAIN, 1, {}), (L.IN_GELU_AFFINE, L.IN_PLAIN, 1, {}), (L.IN_PLAIN, L.IN_UNSHUFFLE, 2, {}), (L.IN_AFFINE, L.IN_UNSHUFFLE, 2, {}),
              (L.IN_PLAIN, L.IN_UNSHUFFLE, 3, {}), (L.IN_PLAIN, L.IN_UNSHUFFLE, 5, {})]
    return m


def pair_cases():
    """(conv row, weight-gradient keyword arguments): the backward pairs ops.py issues -- a TAT conv's (DGELU_SAVED / DSIN | affine
    weight gradient), a block conv's and an up-conv's (PLAIN) -- over the channel and size thresholds."""
    cases = []
    sizes = ((9, 16), (12, 20), (32, 128), (36, 132), (45, 80), (48, 96), (90, 160), (128, 128), (4097, 4), (180, 320), (360, 640))
    for c in CH + (15, 30, 38):
        for H, W in sizes:
            for ep in (L.EP_DGELU_SAVED, L.EP_DSIN):
                for off in ({}, {"x": 4}, {"aux0": 4}):
                    cases.append((conv_row(c, c, H, W, ep_mode=ep, transposed=1, partial=True, off=off), dict(in_mode=L.IN_AFFINE)))
            cases.append((conv_row(c, c, H, W, ep_mode=L.EP_PLAIN, transposed=1), dict(in_mode=L.IN_PLAIN)))
            cases.append((conv_row(4 * c, c, H, W, in_mode=L.IN_UNSHUFFLE, in_s=2, ep_mode=L.EP_PLAIN, transposed=1), dict(in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE, g_s=2)))
    return cases
