"""The case table of the per-family numerical tests (tests/test_conv_family_cases_cpu.py, tests/test_gpu_conv_families.py): one small
case per kernel instantiation that a shipped configuration launches, one per (family, in, ep) pair that only the C ABI reaches, the
NULL variants of every optional pointer, and the k = 5 entry points.  Deterministic, like tests/conv_route_table.py, whose row helpers
it reuses.

The shipped keys are READ from tests/conv_route_pins.json (never copied): for each, `_find` walks a fixed list of small shapes in order of
pixel count and takes the first one on which the host route query (made-up aligned pointers, nothing launched) still names the key's
family and the edge conditions hold -- H no multiple of the family's tile height, a partially filled last tile column behind a full one
with W % 4 == 0, Cout % 16 != 0, Cin % 4 != 0 where the family admits it, B = 2.  A later change of a threshold moves the case to the
next shape that still reaches the family, or, when none is left, fails the coverage test.  Also here: the operands of the two passes."""
import ctypes as C
import functools
import json
import math
import os

import torch

import conv_desc_ref as R
import conv_route_table as T
from boosting_nerv_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_SWITCHES = ("BNERV_SMALL", "BNERV_SPLIT_WIDE_MIN_TILES", "BNERV_PAIR_FUSED", "BNERV_PAIR_FOLD", "BNERV_PAIR_BFW_FILL")
SMALL_FAMS = ("small", "small96")
SPLIT_WGRAD = ("wide_bf16", "wide_f32")                 # the two wide weight-gradient families: the split contract applies

_HS = (5, 6, 9, 10, 13, 17, 18, 21, 25, 33, 37, 45, 65, 69, 129, 133)
_WS = (20, 36, 40, 44, 68, 72, 100, 132, 260)
SHAPES = sorted(((h, w) for h in _HS for w in _WS), key=lambda s: (s[0] * s[1], s))


class _clean_env:
    """The route queries read the BNERV_* switches per call: ask them with the case's switches and nothing else."""

    def __init__(self, env=None):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in ENV_SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in ENV_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.old.items() if v is not None})


def tile_of(fam):
    return (4, 16) if fam in SMALL_FAMS else (8, 32)


def edges(fam, B, Cin, Cout, H, W, vec_rows=True):
    """Which of the edge conditions a shape meets for a family with the given tile."""
    th, tw = tile_of(fam)
    return dict(H=H % th != 0 and H > th, W=W % tw != 0 and W > tw and (W % 4 == 0 or not vec_rows), Cout=Cout % 16 != 0, Cin=Cin % 4 != 0, B=B == 2)


# ---- keys
def conv_key(fam, ints, present):
    return (fam, ints["in_mode"], ints["ep_mode"], ints["k"], ints["in_s"], ints["out_s"], ints["transposed"],
            bool(present["partial"]), bool(present["out2"]), bool(present["aux2"]))


def wgrad_key(fam, ints, present):
    return (fam, ints["k"], ints["in_mode"], ints["g_mode"], ints["g_s"], bool(present["db"]))


def pair_key(form, ci, wi):
    return (form, ci["in_mode"], ci["ep_mode"], ci["k"], ci["in_s"], wi["in_mode"], wi["g_mode"], wi["g_s"])


@functools.lru_cache(None)
def pins():
    with open(os.path.join(HERE, "conv_route_pins.json")) as f:
        return json.load(f)


def pinned_keys(config=None):
    """{kind: {key: the pinned records with that key}} of one configuration (None: all four), in file order."""
    out = {"conv": {}, "wgrad": {}, "pair": {}}
    for cfg, recs in pins().items():
        if config not in (None, cfg):
            continue
        for rec in recs:
            kind, fam = rec[0], rec[-1]
            if kind == "conv":
                key = conv_key(fam, rec[1], {n: n not in rec[2] for n in ("partial", "out2", "aux2")})
            elif kind == "wgrad":
                key = wgrad_key(fam, rec[1], {"db": "db" not in rec[2]})
            else:
                key = pair_key(fam, rec[1], rec[3])
            out[kind].setdefault(key, []).append(rec)
    return out


# ---- route queries on made-up pointers
def conv_family(row, partial=None):
    rows = C.c_int(-7)
    with _clean_env(row["env"]):
        d = T.conv_desc(row, partial=partial)
        fam = L.load().bnerv_conv_family(C.byref(d), C.byref(rows))
        ws = L.load().bnerv_conv_splitk_ws_bytes(C.byref(d))
    return (L.CONV_FAM[fam] if fam >= 0 else "invalid"), rows.value, ws


def wgrad_family(c):
    lib = L.load()
    n = C.c_int(-7)
    with _clean_env(c["env"]):
        ws = lib.bnerv_conv_wgrad_ws_bytes(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["k"])
        d = T.wgrad_desc(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["k"], in_mode=c["in_mode"], g_mode=c["g_mode"], g_s=c["g_s"], ws_bytes=ws)
        fam = lib.bnerv_conv_wgrad_family(C.byref(d), C.byref(n))
    return (L.WGRAD_FAM[fam] if fam >= 0 else "invalid"), n.value


def pair_descs(c):
    """The made-up descriptors of a pair case as ops._wgrad_conv_pair builds them: the weight gradient reads the conv's input as its gradient
    and, for a TAT conv, the epilogue's raw operand as its input; the 1x1 head shares the image too."""
    lib = L.load()
    cv, wg = c["conv"], c["wgrad"]
    cd = T.conv_desc(cv)
    raw = {L.EP_DSIN: cd.aux0, L.EP_DGELU_SAVED: cd.aux1}.get(cv["ep_mode"])
    ws = lib.bnerv_conv_wgrad_ws_bytes(wg["B"], wg["Cin"], wg["Cout"], wg["H"], wg["W"], wg["k"])
    wd = T.wgrad_desc(wg["B"], wg["Cin"], wg["Cout"], wg["H"], wg["W"], wg["k"], in_mode=wg["in_mode"], g_mode=wg["g_mode"], g_s=wg["g_s"], ws_bytes=ws, g=cd.x, x=raw)
    if wg["g_mode"] == L.IN_TANHGRAD:
        wd.gaux = cd.aux0
    return cd, wd


def pair_form(c):
    rows = C.c_int(-7)
    with _clean_env(c["env"]):
        cd, wd = pair_descs(c)
        f = L.load().bnerv_conv_wgrad_pair_form(C.byref(cd), C.byref(wd), C.byref(rows))
    return ("none" if f < 0 else L.PAIR_FORM[f]), rows.value


# ---- the search for a small shape
def _over_records(recs, find_one):
    """The smallest case over the distinct channel counts of a key's pinned records (a key's layers differ in width, and a family may
    start at another image size for each)."""
    best, tried = None, set()
    for rec in recs:
        ch = (rec[1]["Cin"], rec[1]["Cout"])
        if ch in tried:
            continue
        tried.add(ch)
        c = find_one(rec)
        if c is not None:
            v = c["conv"] if c["kind"] == "pair" else c
            rank = (-len(c["edges"]), v["H"] * v["W"])
            if best is None or rank < best[0]:
                best = (rank, c)
    return None if best is None else best[1]


def _units(c0):
    """Channel counts near a shipped one, ragged ones first."""
    seen = []
    for c in (c0 - 1, c0 - 2, c0 - 3, c0 + 1, c0):
        if c > 0 and c not in seen:
            seen.append(c)
    return seen


_RELAX = (("H", "W", "Cout", "Cin", "B"), ("H", "W", "Cout", "B"), ("H", "W", "Cin", "B"), ("H", "W", "B"), ("H", "W"), ())


SHAPES_ODD_W = ((9, 37), (13, 45), (17, 70))             # rows that are not float4-aligned: the scalar forms


def _find(make, fam_of, fam, cin0, cout0, in_s, out_s, max_px=70000, tile_fam=None, shapes=SHAPES):
    """First (fewest pixels, most edge conditions) candidate on which fam_of(candidate) == fam.  make(B, Cin, Cout, H, W) -> candidate."""
    for need in _RELAX:
        for H, W in shapes:
            if H * W > max_px:
                break
            for B in ((2,) if "B" in need else (2, 1)):
                for ci in _units(cin0 // (in_s * in_s)):
                    for co in _units(cout0 // (out_s * out_s)):
                        Cin, Cout = ci * in_s * in_s, co * out_s * out_s
                        e = edges(tile_fam or fam, B, Cin, Cout, H, W, vec_rows=shapes is SHAPES)
                        if not all(e[n] for n in need):
                            continue
                        cand = make(B, Cin, Cout, H, W)
                        if cand is not None and fam_of(cand) == fam:
                            cand["edges"] = sorted(n for n, v in e.items() if v)
                            return cand
    return None


def _conv_case(fam, row, *, bias, out2, aux2, origin):
    c = dict(row, kind="conv", family=fam, bias=bias, out2=out2, aux2=aux2, origin=origin)
    c["key"] = conv_key(fam, c, c)
    return c


def _has_bias(ep):
    return ep in (L.EP_BIAS, L.EP_BIAS_SIN, L.EP_BIAS_RES, L.EP_BIAS_TANH, L.EP_BIAS_GELU)


def _shipped_conv_case(key, rec):
    fam, in_mode, ep, k, in_s, out_s, tr, partial, out2, aux2 = key
    ints = rec[1]

    def make(B, Cin, Cout, H, W):
        row = T.conv_row(Cin, Cout, H, W, k=k, B=B, in_mode=in_mode, ep_mode=ep, in_s=in_s, out_s=out_s, transposed=tr, partial=partial)
        if partial and ep == L.EP_PLAIN and conv_family(row)[2] == 0:       # the shipped call passes a workspace because the library asked for one
            return None
        return row
    row = _find(make, lambda r: conv_family(r)[0], fam, ints["Cin"], ints["Cout"], in_s, out_s)
    if row is None:
        return None
    return _conv_case(fam, row, bias=_has_bias(ep) and "bias" not in rec[2], out2=out2, aux2=aux2, origin="shipped")


# (family, in, ep, out_s) of each family's mode table -- small_modes, q4_modes, wide_modes (the BNERV_CASE table of convbf.hip) and, for
# generic, the pairs ops.py can issue -- with a layer of the family's kind.  Those that no shipped key uses get a case of their own.
# This is a HAND COPY of the kernels' tables: test_every_family_mode_pair_has_a_case checks the cases against this copy, not against csrc/,
# so an (in, ep) pair added to a kernel table needs a line here (a pair removed there fails, because its case stops reaching the family).
# The key stops at (in, ep, out_s): the staged-quad variants of one small-family mode (launch_small_nq: NQ 4 / 8 by Cin <= 16 / 32, 8 / 16
# for the unshuffle prologue) are told apart only by the channel counts of the cases -- the shipped ones bring 13- (NQ 4) and 29-channel
# (NQ 8) inputs and 44- and 60-channel unshuffles (NQ 16); a mode-table case runs the 29- / 60-channel variant alone.
_TAT_C = {"small": (30, 30), "small96": (95, 95), "q4": (11, 10), "wide_bf16": (38, 38), "generic": (30, 30)}
MODE_TABLES = {
    "small": [(L.IN_PLAIN, L.EP_BIAS, 1), (L.IN_PLAIN, L.EP_BIAS, 2), (L.IN_PLAIN, L.EP_BIAS, 3), (L.IN_PLAIN, L.EP_BIAS_SIN, 1), (L.IN_PLAIN, L.EP_BIAS_SIN, 2),
              (L.IN_PLAIN, L.EP_BIAS_SIN, 3), (L.IN_PLAIN, L.EP_BIAS_SIN, 5), (L.IN_PLAIN, L.EP_PLAIN, 1), (L.IN_PLAIN, L.EP_DGELU_SAVED, 1), (L.IN_PLAIN, L.EP_DSIN, 1),
              (L.IN_AFFINE, L.EP_BIAS, 1), (L.IN_AFFINE, L.EP_BIAS_GELU, 1), (L.IN_AFFINE, L.EP_BIAS_RES, 1), (L.IN_UNSHUFFLE, L.EP_PLAIN, 1)],
    "small96": [(L.IN_PLAIN, L.EP_DGELU_SAVED, 1), (L.IN_PLAIN, L.EP_DSIN, 1), (L.IN_AFFINE, L.EP_BIAS_GELU, 1), (L.IN_AFFINE, L.EP_BIAS_RES, 1)],
    "q4": [(L.IN_PLAIN, L.EP_BIAS, 1), (L.IN_PLAIN, L.EP_BIAS_SIN, 1), (L.IN_PLAIN, L.EP_PLAIN, 1), (L.IN_PLAIN, L.EP_DGELU_SAVED, 1), (L.IN_PLAIN, L.EP_DSIN, 1)],
    "wide_bf16": [(L.IN_PLAIN, L.EP_BIAS_SIN, 3), (L.IN_PLAIN, L.EP_BIAS, 3), (L.IN_PLAIN, L.EP_BIAS_SIN, 5), (L.IN_PLAIN, L.EP_BIAS, 5), (L.IN_PLAIN, L.EP_BIAS_SIN, 2),
                  (L.IN_PLAIN, L.EP_BIAS, 2), (L.IN_UNSHUFFLE, L.EP_PLAIN, 1), (L.IN_PLAIN, L.EP_BIAS, 1), (L.IN_PLAIN, L.EP_BIAS_SIN, 1), (L.IN_PLAIN, L.EP_BIAS_TANH, 1),
                  (L.IN_PLAIN, L.EP_PLAIN, 1), (L.IN_AFFINE, L.EP_BIAS, 1), (L.IN_GELU_AFFINE, L.EP_BIAS_RES, 1), (L.IN_PLAIN, L.EP_DSIN, 1),
                  (L.IN_AFFINE, L.EP_BIAS_GELU, 1), (L.IN_AFFINE, L.EP_BIAS_RES, 1), (L.IN_PLAIN, L.EP_DGELU_SAVED, 1)],
    # ops.py on the generic kernels: conv2d_ps / upconv_act (k 1 | 3, any shuffle) and their backward, tat_block, head_tanh (k 1 | 3)
    "generic": [(L.IN_PLAIN, L.EP_BIAS, 1), (L.IN_PLAIN, L.EP_BIAS, 2), (L.IN_PLAIN, L.EP_BIAS_SIN, 2), (L.IN_PLAIN, L.EP_BIAS_TANH, 1), (L.IN_UNSHUFFLE, L.EP_PLAIN, 1),
                (L.IN_TANHGRAD, L.EP_PLAIN, 1), (L.IN_AFFINE, L.EP_BIAS_GELU, 1), (L.IN_GELU_AFFINE, L.EP_BIAS_RES, 1), (L.IN_PLAIN, L.EP_DSIN, 1),
                (L.IN_PLAIN, L.EP_DGELU_SAVED, 1)],
}
_TRANSPOSED_EP = (L.EP_PLAIN, L.EP_DGELU, L.EP_DSIN, L.EP_DGELU_SAVED)


def _mode_case(fam, in_mode, ep, out_s, k=3):
    """A case for (family, in, ep, out_s) on a layer of the family's kind; None when no candidate shape reaches the family."""
    cin0, cout0 = _TAT_C[fam]
    tr = 1 if ep in _TRANSPOSED_EP else 0
    in_s = 2 if (in_mode == L.IN_UNSHUFFLE and fam != "generic") else 1
    if in_mode == L.IN_UNSHUFFLE and fam == "small":
        cin0 = 16                                                               # (x 4: <= 64 gathered channels, a multiple of 4)
    if in_mode == L.IN_TANHGRAD:
        cin0, cout0 = 3, 13
    env = {}
    if fam == "generic":                                                        # the other families switched off or out of reach: odd channel counts, no context
        env = {"BNERV_SMALL": "0"}
    if fam == "wide_bf16":
        env = {"BNERV_SMALL": "0", "BNERV_SPLIT_WIDE_MIN_TILES": "1"}

    def make(B, Cin, Cout, H, W):
        return T.conv_row(Cin, Cout, H, W, k=k, B=B, in_mode=in_mode, ep_mode=ep, in_s=in_s, out_s=out_s, transposed=tr, env=env, ctx=fam != "generic")
    # (the aligned 1x1 head's data gradient is the streaming head kernel: the generic TANHGRAD 1x1 is what rows of odd length run)
    shapes = SHAPES_ODD_W if (in_mode == L.IN_TANHGRAD and k == 1) else SHAPES
    row = _find(make, lambda r: conv_family(r)[0], fam, cin0 * in_s * in_s, cout0 * out_s * out_s, in_s, out_s, shapes=shapes)
    if row is None:
        return None
    return _conv_case(fam, row, bias=_has_bias(ep), out2=ep in (L.EP_BIAS_SIN, L.EP_BIAS_GELU), aux2=ep == L.EP_DSIN, origin="mode table")


def _stem_dgrad_cases():
    """The stem kernel's data gradient stand-alone (in the shipped steps it runs inside the stem pair): an image of <= 256 pixels, long K,
    K-slice slabs in an EP_PLAIN workspace -- gathered through PixelShuffle(5) as the stem up-conv's, and plain."""
    out = []
    # At most 256 pixels, so no shape is ragged in H (> 8 rows) and has a partial 32-column tile behind a full one (>= 36 columns) at once:
    # the gathered case is ragged in H, the plain one in W (test_edge_conditions_per_shipped_key asserts that split).
    for in_mode, in_s, shapes in ((L.IN_UNSHUFFLE, 5, ((9, 20),)), (L.IN_PLAIN, 1, ((6, 36),))):
        def make(B, Cin, Cout, H, W):
            row = T.conv_row(Cin, Cout, H, W, B=B, in_mode=in_mode, ep_mode=L.EP_PLAIN, in_s=in_s, transposed=1, partial=True)
            return row if conv_family(row)[2] > 0 else None
        row = _find(make, lambda r: conv_family(r)[0], "stem_dgrad", 750, 30, in_s, 1, max_px=256, shapes=shapes)
        out.append(None if row is None else _conv_case("stem_dgrad", row, bias=False, out2=False, aux2=False, origin="stem slabs"))
    return out


def _null_variants(c):
    """The other setting of each optional pointer the header lets be NULL.  out2 / aux2 do not take part in the selection: same family.
    An EP_PLAIN workspace does (split-K, the stem's slabs, the 3x3 head's data gradient): the variant is about the family the route names
    for it, which the case records as a fact of the table's build and the CPU test re-asks under the same switches."""
    out = []
    if c["ep_mode"] in (L.EP_BIAS_GELU, L.EP_BIAS_SIN):
        out.append(dict(c, out2=not c["out2"], origin=c["origin"] + ", out2 flipped"))
    if c["ep_mode"] == L.EP_DSIN:
        out.append(dict(c, aux2=not c["aux2"], origin=c["origin"] + ", aux2 flipped"))
    if c["ep_mode"] == L.EP_PLAIN:
        v = dict(c, partial=not c["partial"], origin=c["origin"] + ", partial flipped")
        fam, _, ws = conv_family(v)
        if not (v["partial"] and ws == 0):                  # a workspace the library does not ask for is never passed
            v["family"] = fam
            out.append(v)
    for v in out:
        v["key"] = conv_key(v["family"], v, v)
    return out


def _wgrad_case(fam, B, Cin, Cout, H, W, k, in_mode, g_mode, g_s, db, origin, env=None):
    c = dict(kind="wgrad", family=fam, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=in_mode, g_mode=g_mode, g_s=g_s, db=db, env=dict(env or {}), origin=origin)
    c["key"] = wgrad_key(fam, c, c)
    return c


def _shipped_wgrad_case(key, rec):
    fam, k, in_mode, g_mode, g_s, db = key

    def make(B, Cin, Cout, H, W):
        return _wgrad_case(fam, B, Cin, Cout, H, W, k, in_mode, g_mode, g_s, db, "shipped")
    return _find(make, lambda c: wgrad_family(c)[0], fam, rec[1]["Cin"], rec[1]["Cout"], 1, g_s)


def _shipped_pair_case(key, rec):
    form = key[0]
    ci, wi = rec[1], rec[3]
    partial = "partial" not in rec[2]

    def make(B, Cin, Cout, H, W):
        cv = T.conv_row(Cin, Cout, H, W, k=ci["k"], B=B, in_mode=ci["in_mode"], ep_mode=ci["ep_mode"], in_s=ci["in_s"], out_s=1, transposed=1, partial=partial)
        if partial and ci["ep_mode"] == L.EP_PLAIN and conv_family(cv)[2] == 0:
            return None
        wg = dict(B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=wi["k"], in_mode=wi["in_mode"], g_mode=wi["g_mode"], g_s=wi["g_s"])
        return dict(kind="pair", form=form, conv=cv, wgrad=wg, env={}, aux2="aux2" not in rec[2], origin="shipped", key=key)
    fam_guess = {"q4_lean": "q4", "small_wide": "small", "stem": "small"}.get(form, "generic")      # (only the tile of the edge conditions)
    return _find(make, lambda c: pair_form(c)[0], form, ci["Cin"], ci["Cout"], ci["in_s"], 1, tile_fam=fam_guess)


def _conv5_cases():
    out = []

    def add(Cin, Cout, H, W, **kw):
        c = dict(kind="conv5", B=2, Cin=Cin, Cout=Cout, H=H, W=W, k=5, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS, in_s=1, out_s=1, transposed=0, bias=True, out2=False,
                 aux0=False, env={}, origin="conv5")
        c.update(kw)
        out.append(c)
    for i, out_s in enumerate((1, 2)):
        H, W = ((13, 36), (9, 21))[i]
        for aux0 in (False, True):
            add(7, 19 * out_s * out_s, H, W, out_s=out_s, aux0=aux0)
            add(7, 19 * out_s * out_s, H, W, out_s=out_s, aux0=aux0, ep_mode=L.EP_BIAS_GELU, out2=True)
            add(7, 19 * out_s * out_s, H, W, out_s=out_s, aux0=aux0, ep_mode=L.EP_BIAS_GELU, out2=False)
            add(7, 19 * out_s * out_s, H, W, out_s=out_s, aux0=aux0, ep_mode=L.EP_PLAIN, bias=False)
    for i, in_s in enumerate((1, 2)):                       # the data gradient: gathered (optionally gelu'-weighted) gradient, flipped weight
        H, W = ((9, 36), (13, 21))[i]
        for aux0 in (False, True):
            add(19 * in_s * in_s, 7, H, W, in_s=in_s, in_mode=L.IN_UNSHUFFLE if in_s > 1 else L.IN_PLAIN, transposed=1, aux0=aux0, ep_mode=L.EP_PLAIN, bias=False)
            add(19 * in_s * in_s, 7, H, W, in_s=in_s, in_mode=L.IN_UNSHUFFLE if in_s > 1 else L.IN_PLAIN, transposed=1, aux0=aux0, ep_mode=L.EP_BIAS)
    for i, g_s in enumerate((1, 2)):
        H, W = ((13, 36), (9, 21))[i]
        for gaux in (False, True):
            for db in (True, False):
                out.append(dict(kind="conv5_wgrad", B=2, Cin=7, Cout=19 * g_s * g_s, H=H, W=W, k=5, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE if g_s > 1 else L.IN_PLAIN,
                                g_s=g_s, gaux=gaux, db=db, env={}, origin="conv5"))
    return out


@functools.lru_cache(None)
def build():
    """dict(conv, wgrad, pair, conv5: lists of cases; missing: shipped keys for which no candidate shape reaches the family)."""
    shipped = pinned_keys()
    conv, wgrad, pair, missing = [], [], [], []
    for key, recs in shipped["conv"].items():
        c = _over_records(recs, lambda rec: _shipped_conv_case(key, rec))
        if c is None:
            missing.append(("conv", key))
        else:
            conv.append(c)
    have = {(c["family"], c["in_mode"] if not (c["in_mode"] == L.IN_UNSHUFFLE and c["in_s"] == 1) else L.IN_PLAIN, c["ep_mode"], c["out_s"]) for c in conv}
    for fam, table in MODE_TABLES.items():
        for in_mode, ep, out_s in table:
            for k in ((3, 1) if fam == "generic" and in_mode in (L.IN_PLAIN, L.IN_UNSHUFFLE, L.IN_TANHGRAD) and ep not in (L.EP_DSIN, L.EP_DGELU_SAVED) else (3,)):
                if (fam, in_mode, ep, out_s) in have and k == 3:
                    continue
                c = _mode_case(fam, in_mode, ep, out_s, k)
                if c is None:
                    missing.append(("conv mode", (fam, in_mode, ep, out_s, k)))
                else:
                    conv.append(c)
    for c in _stem_dgrad_cases():
        if c is None:
            missing.append(("conv", "stem_dgrad"))
        else:
            conv.append(c)
    conv += [v for c in list(conv) for v in _null_variants(c)]
    for key, recs in shipped["wgrad"].items():
        c = _over_records(recs, lambda rec: _shipped_wgrad_case(key, rec))
        if c is None:
            missing.append(("wgrad", key))
            continue
        wgrad.append(c)
        v = dict(c, db=not c["db"], origin="shipped, db flipped")
        v["key"] = wgrad_key(v["family"], v, v)
        wgrad.append(v)
    for key, recs in shipped["pair"].items():
        if key[0] == "none":                                # covered by its two stand-alone halves
            continue
        c = _over_records(recs, lambda rec: _shipped_pair_case(key, rec))
        if c is None:
            missing.append(("pair", key))
        else:
            pair.append(c)
    seen, uniq = set(), []
    for c in conv:                                          # a flipped variant may coincide with another shipped key's case
        ident = (c["key"], c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["bias"], tuple(sorted(c["env"].items())))
        if ident not in seen:
            seen.add(ident)
            uniq.append(c)
    return dict(conv=uniq, wgrad=wgrad, pair=pair, conv5=_conv5_cases(), missing=missing)


def case_id(c):
    if c["kind"] == "pair":
        v = c["conv"]
        return f"{c['form']}-in{v['in_mode']}s{v['in_s']}-ep{v['ep_mode']}-{v['B']}x{v['Cin']}x{v['Cout']}x{v['H']}x{v['W']}"
    s = f"{c.get('family', c['kind'])}-k{c['k']}-in{c['in_mode']}"
    if c["kind"] in ("conv", "conv5"):
        s += f"s{c['in_s']}-ep{c['ep_mode']}s{c['out_s']}" + ("-T" if c["transposed"] else "") + ("-ws" if c.get("partial") else "")
        s += ("-out2" if c["out2"] else "") + ("-aux2" if c.get("aux2") else "") + ("-aux0" if c.get("aux0") else "")
    else:
        s += f"-g{c['g_mode']}s{c['g_s']}" + ("-db" if c["db"] else "") + ("-gaux" if c.get("gaux") else "")
    return s + f"-{c['B']}x{c['Cin']}x{c['Cout']}x{c['H']}x{c['W']}"


# ---- operands
def _gen(c, salt):
    return torch.Generator().manual_seed(hash_of(case_id(c)) + salt)


def hash_of(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def _ints(gen, shape, lo, hi, q=1.0):
    return torch.randint(lo, hi + 1, shape, generator=gen).float() * q


def _conv_shapes(c):
    si, so = c["in_s"], c["out_s"]
    B, Cin, Cout, H, W, k = (c[n] for n in ("B", "Cin", "Cout", "H", "W", "k"))
    wsh = (Cin, Cout, k, k) if c["transposed"] else (Cout, Cin, k, k)
    xs = (B, Cin // (si * si), H * si, W * si) if c["in_mode"] == L.IN_UNSHUFFLE else (B, Cin, H, W)
    return xs, wsh, (B, Cout, H, W), (B, Cout // (so * so), H * so, W * so)


def conv_operands(c, exact):
    """CPU f32 operands of a conv / conv5 case by descriptor pointer name (absent = NULL).  exact: small dyadic values (integers in [-3, 3],
    weights in eighths, bias / shift / aux in halves, scale in {-1/2, 0, 1/2, 1}); otherwise seeded normals with weights scaled by
    1 / sqrt(Cin k^2) and a distinct scale per (b, c).  (No case needed a narrower range to pass the operand check.)"""
    gen = _gen(c, 1 if exact else 2)
    xs, wsh, cs, _ = _conv_shapes(c)
    B, Cin, Cout, k, ep, im = c["B"], c["Cin"], c["Cout"], c["k"], c["ep_mode"], c["in_mode"]
    half = (lambda *sh: _ints(gen, sh, -4, 4, 0.5)) if exact else (lambda *sh: torch.randn(*sh, generator=gen))
    t = {}
    if exact:
        t["x"] = _ints(gen, xs, -3, 3)
        t["w"] = _ints(gen, wsh, -4, 4, 0.125)
        scale = lambda n: torch.tensor([-0.5, 0.0, 0.5, 1.0])[torch.randint(0, 4, (B, n), generator=gen)]
    else:
        t["x"] = torch.randn(*xs, generator=gen)
        t["w"] = torch.randn(*wsh, generator=gen) / math.sqrt(Cin * k * k)
        scale = lambda n: torch.randn(B, n, generator=gen) * 0.5
    if c.get("bias"):
        t["bias"] = half(Cout)
    if im in (L.IN_AFFINE, L.IN_GELU_AFFINE):
        t["scale"], t["shift"] = scale(Cin), half(B, Cin)
    if im == L.IN_TANHGRAD:
        t["aux0"] = _ints(gen, xs, 0, 4, 0.25) if exact else torch.rand(*xs, generator=gen)
    if c["kind"] == "conv5":
        if c["aux0"]:
            t["aux0"] = _ints(gen, xs, -2, 2, 0.5) if exact else torch.randn(*xs, generator=gen)
        return t
    if ep == L.EP_BIAS_RES:
        t["aux0"] = half(*cs)
    if ep in (L.EP_DGELU, L.EP_DGELU_SAVED, L.EP_DSIN):
        t["scale"] = scale(Cout)
        t["aux0"], t["aux1"] = half(*cs), half(*cs)
        if ep == L.EP_DGELU:
            del t["aux1"]
        if ep == L.EP_DSIN and c["aux2"]:
            t["aux2"] = half(*cs)
    return t


def wgrad_operands(c, exact):
    gen = _gen(c, 3 if exact else 4)
    B, Cin, Cout, H, W, s = c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["g_s"]
    gs = (B, Cout // (s * s), H * s, W * s) if c["g_mode"] == L.IN_UNSHUFFLE else (B, Cout, H, W)
    t = {}
    if exact:
        t["x"], t["g"] = _ints(gen, (B, Cin, H, W), -3, 3), _ints(gen, gs, -3, 3)
    else:
        t["x"], t["g"] = torch.randn(B, Cin, H, W, generator=gen), torch.randn(*gs, generator=gen)
    if c["in_mode"] in (L.IN_AFFINE, L.IN_GELU_AFFINE):
        if exact:
            t["scale"] = torch.tensor([-0.5, 0.0, 0.5, 1.0])[torch.randint(0, 4, (B, Cin), generator=gen)]
            t["shift"] = _ints(gen, (B, Cin), -4, 4, 0.5)
        else:
            t["scale"], t["shift"] = torch.randn(B, Cin, generator=gen) * 0.5, torch.randn(B, Cin, generator=gen)
    if c["g_mode"] == L.IN_TANHGRAD:
        t["gaux"] = _ints(gen, gs, 0, 4, 0.25) if exact else torch.rand(*gs, generator=gen)
    if c["kind"] == "conv5_wgrad" and c["gaux"]:
        t["gaux"] = _ints(gen, gs, -2, 2, 0.5) if exact else torch.randn(*gs, generator=gen)
    return t


def pair_operands(c, exact):
    """(conv operands, weight-gradient operands) of a pair, sharing what ops._wgrad_conv_pair shares: g = the conv's x; the weight gradient's
    x = the TAT epilogue's raw operand (aux0 of EP_DSIN, aux1 of EP_DGELU_SAVED), its scale = the conv's; the 1x1 head's gaux = the conv's aux0."""
    cv = dict(c["conv"], kind="conv", bias=False, out2=False, aux2=c["aux2"])
    cv["family"] = "pair"
    tc = conv_operands(dict(cv, key=None), exact)
    wg = dict(c["wgrad"], kind="wgrad", family="pair", db=True, env={})
    tw = wgrad_operands(wg, exact)
    tw["g"] = tc["x"]
    ep = cv["ep_mode"]
    if ep in (L.EP_DSIN, L.EP_DGELU_SAVED):
        tw["x"] = tc["aux0"] if ep == L.EP_DSIN else tc["aux1"]
        tw["scale"] = tc["scale"]
    if wg["g_mode"] == L.IN_TANHGRAD:
        tw["gaux"] = tc["aux0"]
    return cv, tc, wg, tw


# ---- references, exactness classes and the random pass's allowance
SPLIT_BOUND = 3.5e-7            # tools/split_contract.py: the stated f32 contract of the split-bf16 kernels, relative to sum |a| |b|
SIN_TOL, GELU_TOL, DGELU_TOL = 3e-7, 3e-7, 6e-7         # test_sincos_epilogue_accuracy / test_gelu_pair_epilogue_accuracy
U = 2.0 ** -24
LINEAR_EP = (L.EP_BIAS, L.EP_PLAIN, L.EP_BIAS_RES, L.EP_DGELU_SAVED, L.EP_DSIN)


def reference(c, t, **kw):
    return {"conv": R.conv_ref, "conv5": R.conv5_ref, "wgrad": R.wgrad_ref, "conv5_wgrad": R.conv5_wgrad_ref}[c["kind"]](c, t, **kw)


def pre_exact(c):
    """The conv result v (and bias sum u) of the exact pass is exactly representable: every prologue but gelu."""
    return c["in_mode"] != L.IN_GELU_AFFINE


def out_exact(c):
    return pre_exact(c) and (c["kind"] in ("wgrad", "conv5_wgrad") or c["ep_mode"] in LINEAR_EP)


def coeff(c, split, sums=False):
    """Relative error allowed per unit of sum |a| |b|: the split contract, or the worst case of an f32 chain of K_eff terms (K_eff: Cin k^2,
    B H W for a weight gradient, Cin k^2 + H W for the per-channel sums of a d-epilogue, which contract over taps and pixels)."""
    if split:
        return SPLIT_BOUND
    k_eff = c["B"] * c["H"] * c["W"] if c["kind"] in ("wgrad", "conv5_wgrad") else c["Cin"] * c["k"] ** 2 + (c["H"] * c["W"] if sums else 0)
    return (k_eff + 2) * U


def tanhgrad_rounding(x):
    """The ONE rounding term of the random pass, applied to the IN_TANHGRAD prologue of the conv cases only.  tanh' = 0.5 (1 - (2 img - 1)^2)
    is a difference of numbers up to 1, so evaluated in f32 its error is absolute (three roundings, 3 * 2^-24) where the factor itself is near
    0: relative to |a| it is unbounded, and sum |a| |W| cannot pay for it.  The case that needs it is the generic 1x1 tanh-grad data
    gradient with K = 2 (2x2x12x9x37): without the term its worst error is 2.6 times (K + 2) 2^-24 sum |a| |W|.  No split family has this prologue."""
    return 3 * U * x.double().abs()


def conv_allowance(c, t, r, split, exact_pre=False):
    """Per-element allowance of the random pass for out / out2 / sums of a conv case, nothing beyond what the contract names:
        coeff * S,  S = sum |a| |W| + |bias| (+ |aux0| of EP_BIAS_RES, + |aux1| of EP_DSIN after the slope): bias and residual are folded into
        the sum under the same coefficient, as tools/split_contract.py does;
        times the epilogue's slope bound (1 sin, 1.13 gelu and gelu', |1 + scale| |aux| for the d-epilogues);
        plus the function bound of a non-linear epilogue or prologue (sin 3e-7, gelu 3e-7 (1 + |u|), gelu' 6e-7, gelu(x) carried through |W|);
        plus tanhgrad_rounding for IN_TANHGRAD (see there) -- the only rounding term.
    The (ds, dt) sums contract over taps and pixels: coeff(sums) * sum_p S_v |aux|.  r: the float64 reference of the same operands.  tanh has no
    function bound in the project: out is None there (the caller applies the forward tolerance of close()).  exact_pre: the exact pass, where
    v and u are exact and only the function's own error is left."""
    conv2d, shuffle = torch.nn.functional.conv2d, torch.nn.functional.pixel_shuffle
    ab = reference(c, t, absolute=True)
    f64 = lambda n: None if t.get(n) is None else t[n].double()
    sv = ab["v"]                                             # sum |a| |W|
    extra = 0                                               # absolute terms carried through |W|
    if c["in_mode"] == L.IN_GELU_AFFINE:                    # gelu(x) off by <= GELU_TOL (1 + |x|), carried through |1 + scale| and |W|
        da = GELU_TOL * (1 + t["x"].double().abs()) * (1 + f64("scale")).abs()[:, :, None, None]
        extra = conv2d(da, ab["weff"], padding=(c["k"] - 1) // 2)
    if c["in_mode"] == L.IN_TANHGRAD:
        extra = conv2d(tanhgrad_rounding(t["x"]), ab["weff"], padding=(c["k"] - 1) // 2)
    ep = c["ep_mode"]
    bias = 0 if f64("bias") is None else f64("bias")[None, :, None, None].abs()
    k, ks = coeff(c, split), coeff(c, split, sums=True)
    if exact_pre:
        k = ks = 0.0
        extra = 0
    pre = k * (sv + bias) + extra
    res = dict(out2=None, sums=None)
    if ep in (L.EP_PLAIN, L.EP_BIAS):
        out = pre
    elif ep == L.EP_BIAS_RES:
        out = k * (sv + bias + f64("aux0").abs()) + extra
    elif ep == L.EP_BIAS_SIN:
        out = pre + SIN_TOL
        res["out2"] = pre + SIN_TOL
    elif ep == L.EP_BIAS_TANH:
        out = None
    elif ep == L.EP_BIAS_GELU:
        out = 1.13 * pre + GELU_TOL * (1 + r["mid"]["u"].abs())
        res["out2"] = 1.13 * pre + DGELU_TOL
    else:
        s1 = (1 + f64("scale")).abs()[:, :, None, None]
        if ep == L.EP_DSIN:
            gate = 1 if f64("aux2") is None else f64("aux2").abs()
            out = (k * (sv * s1 + f64("aux1").abs()) + extra * s1) * gate
            mult, mult_tol = f64("aux0").abs(), 0
        elif ep == L.EP_DGELU_SAVED:
            out = (k * sv + extra) * s1 * f64("aux0").abs()
            mult, mult_tol = f64("aux1").abs(), 0
        else:
            out = (k * sv + extra) * s1 * R.gelu_grad(f64("aux0")).abs() + DGELU_TOL * r["mid"]["vs"].abs()
            mult, mult_tol = R.gelu(f64("aux0")).abs(), GELU_TOL * (1 + f64("aux0").abs())
        pix = ks * sv + extra
        res["sums"] = torch.stack([(pix * mult + r["v"].abs() * mult_tol).sum((2, 3)), pix.sum((2, 3))], 1)
    if c["out_s"] > 1 and out is not None:
        out = shuffle(out, c["out_s"])
        res["out2"] = None if res["out2"] is None else shuffle(res["out2"], c["out_s"])
    res["out"] = out
    return res


def wgrad_allowance(c, t, split):
    """dw: coeff * sum |g| |a| (+ the gelu bound of IN_GELU_AFFINE carried through |g|); db: coeff * sum |g|.  split: 3.5e-7 for both."""
    ab = reference(c, t, absolute=True)
    k = coeff(c, split)
    extra = 0
    if c["in_mode"] == L.IN_GELU_AFFINE:
        da = GELU_TOL * (1 + t["x"].double().abs()) * (1 + t["scale"].double()).abs()[:, :, None, None]
        cols = torch.nn.functional.unfold(da, c["k"], padding=(c["k"] - 1) // 2)
        extra = torch.einsum("bop,bkp->ok", ab["g"].flatten(2), cols).reshape(ab["dw"].shape)
    return dict(dw=k * ab["dw"] + extra, db=k * ab["db"])
