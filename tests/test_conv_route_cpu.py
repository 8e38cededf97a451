"""CPU tests of the kernel selection of the conv entry points (csrc/route.h) through the host queries: the three
long-standing ones (bnerv_conv_partial_rows, bnerv_conv_splitk_ws_bytes, bnerv_conv_wgrad_ws_bytes) answer what the commit before the
routes answered (tests/conv_route_answers.json, recorded from that commit's library by tools/record_conv_route.py over
tests/conv_route_table.py), and the three route queries are consistent with them on every row.  Made-up pointers: nothing is launched."""
import ctypes as C
import json
import os

import pytest

import conv_route_table as T
from boosting_nerv_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
FAM = {n: i for i, n in enumerate(L.CONV_FAM)}
WFAM = {n: i for i, n in enumerate(L.WGRAD_FAM)}
FORM = {n: i for i, n in enumerate(L.PAIR_FORM)}
SMALL_FAMS = (FAM["small"], FAM["small96"])


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "conv_route_answers.json")) as f:
        return json.load(f)


def _small_tiles(H, W):
    return ((H + 3) // 4) * ((W + 15) // 16)


def _family(lib, d):
    rows = C.c_int(-7)
    return lib.bnerv_conv_family(C.byref(d), C.byref(rows)), rows.value


def _set_env(monkeypatch, env):
    for k in ("BNERV_SMALL", "BNERV_SPLIT_WIDE_MIN_TILES", "BNERV_PAIR_FUSED", "BNERV_PAIR_FOLD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_the_three_existing_queries_answer_what_the_parent_commit_answered(recorded, monkeypatch):
    lib = L.load()
    rows = T.conv_rows()
    assert len(rows) == len(recorded["conv"]) > 300
    bad = []
    for i, (r, want) in enumerate(zip(rows, recorded["conv"])):
        _set_env(monkeypatch, r["env"])
        d = T.conv_desc(r)
        got = [lib.bnerv_conv_partial_rows(C.byref(d)), lib.bnerv_conv_splitk_ws_bytes(C.byref(d))]
        if got != want:
            bad.append((i, r, got, want))
    assert not bad, bad[:5]
    dims = T.wgrad_dims()
    assert len(dims) == len(recorded["wgrad_ws_bytes"])
    bad = [(d, lib.bnerv_conv_wgrad_ws_bytes(*d), want) for d, want in zip(dims, recorded["wgrad_ws_bytes"]) if lib.bnerv_conv_wgrad_ws_bytes(*d) != want]
    assert not bad, bad[:5]


def test_conv_family_and_rows_are_one_decision_on_every_row(monkeypatch):
    """rows of the family query == bnerv_conv_partial_rows; 4x16 tiles exactly for the low-resolution families, bnerv_conv_tiles otherwise;
    for the sums epilogues neither depends on `partial`; a split-K / stem workspace is asked for exactly where the family writes one."""
    lib = L.load()
    seen = set()
    for i, r in enumerate(T.conv_rows()):
        _set_env(monkeypatch, r["env"])
        d = T.conv_desc(r)
        fam, rows = _family(lib, d)
        seen.add(fam)
        assert 0 <= fam < len(L.CONV_FAM), (i, r, fam)
        assert rows == lib.bnerv_conv_partial_rows(C.byref(d)), (i, r)
        assert rows == (_small_tiles(r["H"], r["W"]) if fam in SMALL_FAMS else lib.bnerv_conv_tiles(r["H"], r["W"])), (i, r, fam, rows)
        if r["env"].get("BNERV_SMALL") == "0":
            assert fam not in SMALL_FAMS, (i, r)
        if r["ep_mode"] in T.SUMS:
            assert _family(lib, T.conv_desc(r, partial=not r["partial"])) == (fam, rows), (i, r)
        ws = lib.bnerv_conv_splitk_ws_bytes(C.byref(d))
        if r["ep_mode"] != L.EP_PLAIN:
            assert ws == 0, (i, r)
        else:       # with the workspace the query asks for, the launch runs a family that uses it (and the head / low-resolution kernels want none)
            fam_ws, _ = _family(lib, T.conv_desc(r, partial=True))
            assert ws == 0 or fam_ws in (FAM["stem_dgrad"], FAM["wide_bf16"], FAM["generic"]), (i, r, ws, fam_ws)
            assert ws > 0 or fam_ws != FAM["stem_dgrad"], (i, r)
            if fam_ws == FAM["stem_dgrad"]:
                assert ws == ((r["Cin"] + 7) // 8) * r["B"] * r["Cout"] * r["H"] * r["W"] * 4 and r["H"] * r["W"] <= 256, (i, r)
            if not r["partial"]:
                assert fam != FAM["stem_dgrad"], (i, r)
    assert seen == set(range(len(L.CONV_FAM))), "the table reaches every family"


def test_families_of_layers_on_either_side_of_the_thresholds(monkeypatch):
    lib = L.load()
    _set_env(monkeypatch, {})
    fam = lambda *a, **kw: L.CONV_FAM[_family(lib, T.conv_desc(T.conv_row(*a, **kw)))[0]]
    assert fam(12, 12, 64, 64) == "q4" and fam(8, 12, 64, 64) == "generic" and fam(13, 12, 64, 64) == "small" and fam(12, 13, 64, 64) == "small"
    assert fam(13, 12, 720, 1280) == "generic" and fam(12, 12, 64, 62) == "generic" and fam(12, 12, 64, 64, off={"x": 4}) == "generic"
    assert fam(30, 30, 128, 128) == "small" and fam(30, 30, 4097, 4) == "wide_bf16" and fam(30, 30, 4097, 4, ctx=False) == "generic"
    assert fam(32, 30, 32, 32) == "small" and fam(33, 30, 64, 128) == "wide_bf16" and fam(33, 30, 32, 32) == "generic"      # (4 tiles < 16)
    tat = dict(in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_GELU)
    assert fam(95, 95, 9, 16, **tat) == "small96" and fam(96, 96, 32, 32, **tat) == "small96" and fam(97, 97, 32, 32, **tat) == "generic"
    assert fam(95, 95, 257, 4, **tat) == "wide_bf16" and fam(95, 95, 9, 16) == "generic"                                      # (no 96-channel form of EP_BIAS)
    assert fam(12, 48, 180, 320, ep_mode=L.EP_BIAS_SIN, out_s=2) == "small" and fam(12, 48, 16385, 4, ep_mode=L.EP_BIAS_SIN, out_s=2) == "wide_bf16"
    up = dict(in_mode=L.IN_UNSHUFFLE, in_s=2, ep_mode=L.EP_PLAIN, transposed=1)
    assert fam(48, 12, 180, 320, **up) == "small" and fam(64, 16, 90, 160, **up) == "small" and fam(68, 17, 90, 160, **up) == "wide_bf16"
    assert fam(12, 3, 64, 64, k=1, ep_mode=L.EP_BIAS_TANH) == "head1_fwd" and fam(12, 3, 64, 63, k=1, ep_mode=L.EP_BIAS_TANH) == "generic"
    assert fam(3, 12, 64, 64, k=1, in_mode=L.IN_TANHGRAD, ep_mode=L.EP_PLAIN, transposed=1) == "head1_dgrad"
    assert fam(38, 3, 64, 64, ep_mode=L.EP_BIAS_TANH) == "head3" and fam(38, 3, 1023, 4, ep_mode=L.EP_BIAS_TANH) == "wide_bf16"
    dg = dict(ep_mode=L.EP_PLAIN, transposed=1)
    assert fam(750, 30, 9, 16, partial=True, **dg) == "stem_dgrad" and fam(750, 30, 9, 16, **dg) == "generic"
    assert fam(750, 30, 13, 20, partial=True, **dg) == "generic" and fam(127, 30, 9, 16, partial=True, **dg) == "generic"
    monkeypatch.setenv("BNERV_SMALL", "0")
    assert fam(30, 30, 32, 32) == "generic" and fam(30, 30, 32, 128) == "wide_bf16" and fam(30, 30, 32, 96) == "generic"
    monkeypatch.setenv("BNERV_SPLIT_WIDE_MIN_TILES", "12")
    assert fam(30, 30, 32, 96) == "wide_bf16"


def test_the_3x3_head_data_gradient_reports_its_own_family_and_no_low_resolution_rows(recorded, monkeypatch):
    """The named exception to "the parent's answers": conv_route_table.changed_rows().  A 3 -> C data gradient with EP_PLAIN and no
    workspace on an image of 4096..16384 pixels runs on the head kernel (which writes no rows); the old query named the 4x16 tiles of the
    low-resolution family, which takes the layer only when a workspace is passed.  The old answers are in the recorded file; the new
    answer follows the launch, so for EP_PLAIN -- and only there -- it reads `partial`."""
    lib = L.load()
    _set_env(monkeypatch, {})
    rows = T.changed_rows()
    assert len(rows) == len(recorded["conv_changed"]) > 0
    for r, (old_rows, old_ws) in zip(rows, recorded["conv_changed"]):
        assert r["ep_mode"] == L.EP_PLAIN and not r["partial"]
        assert old_rows == _small_tiles(r["H"], r["W"]) != lib.bnerv_conv_tiles(r["H"], r["W"]), r       # what the parent said
        assert _family(lib, T.conv_desc(r)) == (FAM["head3"], lib.bnerv_conv_tiles(r["H"], r["W"])), r
        assert _family(lib, T.conv_desc(r, partial=True)) == (FAM["small"], old_rows), r               # with a workspace: the parent's answer
        assert lib.bnerv_conv_splitk_ws_bytes(C.byref(T.conv_desc(r))) == old_ws, r


def test_weight_gradient_family_and_slabs_fit_the_mode_free_workspace():
    lib = L.load()
    seen = set()
    for dims in T.wgrad_dims():
        B, Cin, Cout, H, W, k = dims
        ws = lib.bnerv_conv_wgrad_ws_bytes(*dims)
        for in_mode, g_mode, g_s, off in T.wgrad_modes(k):
            if Cout % (g_s * g_s):
                continue
            n = C.c_int(-7)
            fam = lib.bnerv_conv_wgrad_family(C.byref(T.wgrad_desc(*dims, in_mode=in_mode, g_mode=g_mode, g_s=g_s, off=off, ws_bytes=ws)), C.byref(n))
            seen.add(fam)
            assert 0 <= fam < len(L.WGRAD_FAM), (dims, fam)
            assert (n.value == 0) == (fam == WFAM["stem"]) and n.value * Cout * (Cin * k * k + 1) * 4 <= ws, (dims, in_mode, g_mode, g_s, fam, n.value, ws)
            if off:                                         # rows that are not 16-byte aligned: the scalar form only
                assert fam in (WFAM["generic"], WFAM["stem"]), (dims, off, fam)
    assert seen == set(range(len(L.WGRAD_FAM)))
    fam = lambda *d, **kw: L.WGRAD_FAM[lib.bnerv_conv_wgrad_family(C.byref(T.wgrad_desc(*d, **kw)), None)]
    assert fam(1, 12, 12, 64, 64, 3) == "lean" and fam(1, 13, 12, 64, 64, 3) == "wide_f32" and fam(1, 12, 16, 64, 64, 3) == "lean"
    assert fam(1, 12, 17, 64, 64, 3) == "wide_bf16" and fam(1, 12, 17, 32, 96, 3) == "wide_f32" and fam(1, 12, 17, 64, 62, 3) == "generic"
    assert fam(1, 15, 3, 64, 64, 1) == "lean" and fam(1, 16, 16, 64, 64, 1) == "gemm1x1" and fam(1, 16, 16, 36, 64, 1) == "generic"
    assert fam(1, 30, 64, 9, 16, 3) == "stem" and fam(1, 30, 63, 9, 16, 3) == "wide_f32" and fam(1, 30, 64, 13, 20, 3) == "wide_f32"
    assert fam(1, 12, 12, 64, 64, 3, in_mode=L.IN_AFFINE, g_mode=L.IN_UNSHUFFLE, g_s=2) == "generic"      # (no lean instantiation)


def _pair(lib, r, wkw):
    """The (conv, weight-gradient) descriptors of one backward pair as ops._wgrad_conv_pair builds them: the weight gradient reads the
    conv's input as its gradient and, for a TAT conv, the epilogue's raw operand as its input."""
    cd = T.conv_desc(r)
    raw = cd.aux0 if r["ep_mode"] == L.EP_DSIN else cd.aux1
    Cin, Cout = r["Cout"], r["Cin"]
    ws = lib.bnerv_conv_wgrad_ws_bytes(r["B"], Cin, Cout, r["H"], r["W"], 3)
    return cd, T.wgrad_desc(r["B"], Cin, Cout, r["H"], r["W"], 3, ws_bytes=ws, g=cd.x, x=raw, **wkw)


def test_a_pair_form_writes_the_rows_the_caller_sized_or_is_not_taken(monkeypatch):
    lib = L.load()
    seen = set()
    for env in ({}, {"BNERV_PAIR_FUSED": "8"}, {"BNERV_SMALL": "0"}):
        _set_env(monkeypatch, env)
        for r, wkw in T.pair_cases():
            cd, wd = _pair(lib, r, wkw)
            rows = C.c_int(-7)
            form = lib.bnerv_conv_wgrad_pair_form(C.byref(cd), C.byref(wd), C.byref(rows))
            seen.add(form)
            assert -1 <= form < len(L.PAIR_FORM), (r, form)
            if form == -1:
                assert rows.value == 0
                continue
            fam, fam_rows = _family(lib, cd)
            if r["ep_mode"] in T.SUMS:
                assert rows.value == lib.bnerv_conv_partial_rows(C.byref(cd)), (env, r, form)
            # with the shipped tables every form pairs the family the stand-alone launch runs -- except the wide form, which takes the
            # up-conv data gradients (EP_PLAIN: no rows) that stand alone on the low-resolution family
            want = {FORM["q4_lean"]: ("q4",), FORM["small_wide"]: ("small",), FORM["bf16_wide"]: ("wide_bf16", "small")}[form]
            assert L.CONV_FAM[fam] in want, (env, r, form, fam)
            if form == FORM["bf16_wide"]:
                assert r["ep_mode"] == L.EP_PLAIN
    assert {FORM["q4_lean"], FORM["small_wide"], FORM["bf16_wide"], -1} <= seen


def test_pair_forms_of_known_pairs(monkeypatch):
    lib = L.load()
    _set_env(monkeypatch, {})

    def form(r, **wkw):
        cd, wd = _pair(lib, r, wkw)
        rows = C.c_int()
        f = lib.bnerv_conv_wgrad_pair_form(C.byref(cd), C.byref(wd), C.byref(rows))
        return ("none" if f < 0 else L.PAIR_FORM[f]), rows.value
    tat = lambda c, H, W, ep=L.EP_DGELU_SAVED, **kw: T.conv_row(c, c, H, W, ep_mode=ep, transposed=1, partial=True, **kw)
    assert form(tat(12, 48, 96), in_mode=L.IN_AFFINE) == ("q4_lean", 6 * 3)
    assert form(tat(15, 9, 16), in_mode=L.IN_AFFINE) == ("small_wide", 3) and form(tat(15, 12, 20, L.EP_DSIN), in_mode=L.IN_AFFINE) == ("small_wide", 3 * 2)
    assert form(tat(30, 32, 128), in_mode=L.IN_AFFINE) == ("small_wide", 8 * 8) and form(tat(30, 36, 132, L.EP_DSIN), in_mode=L.IN_AFFINE) == ("small_wide", 9 * 9)
    assert form(tat(30, 9, 16), in_mode=L.IN_AFFINE) == ("none", 0)                       # (2 tiles: the f32 wide weight gradient has no 30-channel pair)
    assert form(tat(12, 48, 96, off={"x": 4}), in_mode=L.IN_AFFINE) == ("none", 0)
    up = lambda c, H, W: T.conv_row(4 * c, c, H, W, in_mode=L.IN_UNSHUFFLE, in_s=2, ep_mode=L.EP_PLAIN, transposed=1)
    assert form(up(12, 180, 320), g_mode=L.IN_UNSHUFFLE, g_s=2)[0] == "bf16_wide" and form(up(12, 90, 160), g_mode=L.IN_UNSHUFFLE, g_s=2)[0] == "small_wide"
    # the stem stage and the 1x1 head
    stem = T.conv_row(128, 32, 8, 16, in_mode=L.IN_UNSHUFFLE, in_s=2, ep_mode=L.EP_PLAIN, transposed=1, partial=True)
    assert form(stem, g_mode=L.IN_UNSHUFFLE, g_s=2)[0] == "stem"
    stem["partial"] = False
    assert form(stem, g_mode=L.IN_UNSHUFFLE, g_s=2)[0] != "stem"
    head = T.conv_row(3, 12, 64, 64, k=1, in_mode=L.IN_TANHGRAD, ep_mode=L.EP_PLAIN, transposed=1)
    cd = T.conv_desc(head)
    ws = lib.bnerv_conv_wgrad_ws_bytes(1, 12, 3, 64, 64, 1)
    wd = T.wgrad_desc(1, 12, 3, 64, 64, 1, g_mode=L.IN_TANHGRAD, ws_bytes=ws, g=cd.x)
    wd.gaux = cd.aux0
    assert lib.bnerv_conv_wgrad_pair_form(C.byref(cd), C.byref(wd), None) == FORM["head"]


# ---- the shipped layers.  tests/conv_route_pins.json: every distinct conv, weight-gradient and pair call of one training step of c1
# (NeRV-boost 720p), c3 (HNeRV-boost 1080p), c4 (E-NeRV-boost 1080p) and the HNeRV baseline (720p) -- integer fields, which pointers are
# NULL, which pointers of a pair are the same tensor -- with the family / form each runs on.  The families are those of the kernel names in
# the recorded traces (profiles/ops_plumbing.md: c1; profiles/r06_timeline_c3.md, r06_timeline_c4.md; profiles/hnerv_baseline.md).
# The file is a RECORDING of the library at the change that introduced the routes (tools/record_route_pins.py asks the three route
# queries, i.e. the code under test), so by itself it pins against regressions only.  The yardstick it was checked against is the traces:
# per configuration, the number of calls of each family equals the number of launches of that family's kernel names in one traced step
# (the table in profiles/conv_route.md).
def _pinned_desc(cls, ints, nulls, base, alias=None):
    alias = alias or {}
    vals = []
    for i, (n, t) in enumerate(cls._fields_):
        if t is C.c_void_p:
            vals.append(None if n in nulls else C.c_void_p(alias.get(n) or T._p(base + i)))
        else:
            vals.append(ints[n])
    return cls(*vals)


@pytest.mark.parametrize("config", ["c1", "c3", "c4", "hnerv"])
def test_families_of_the_shipped_layers(config, monkeypatch):
    lib = L.load()
    _set_env(monkeypatch, {})
    with open(os.path.join(HERE, "conv_route_pins.json")) as f:
        pins = json.load(f)[config]
    kinds = set()
    for rec in pins:
        kind, want = rec[0], rec[-1]
        kinds.add((kind, want))
        if kind == "conv":
            got = L.CONV_FAM[lib.bnerv_conv_family(C.byref(_pinned_desc(L.ConvDesc, rec[1], rec[2], 0)), None)]
        elif kind == "wgrad":
            got = L.WGRAD_FAM[lib.bnerv_conv_wgrad_family(C.byref(_pinned_desc(L.WgradDesc, rec[1], rec[2], 32)), None)]
        else:
            cd = _pinned_desc(L.ConvDesc, rec[1], rec[2], 0)
            alias = {wn: getattr(cd, cn) for cn, wn in rec[5]}
            alias["ctx"] = cd.ctx
            f = lib.bnerv_conv_wgrad_pair_form(C.byref(cd), C.byref(_pinned_desc(L.WgradDesc, rec[3], rec[4], 32, alias)), None)
            got = "none" if f < 0 else L.PAIR_FORM[f]
        assert got == want, (config, rec)
    if config == "c3":      # the encoder's pointwise weight gradients: wgrad1x1_kernel at 216x384 and above, conv_wgrad_kernel<1, ...> on the small images
        assert ("wgrad", "gemm1x1") in kinds and ("wgrad", "generic") in kinds and ("conv", "small96") in kinds and ("conv", "head3") in kinds
    if config == "c1":      # every form of the pair, and both low-resolution roles, are in the flagship step
        assert {("pair", f) for f in L.PAIR_FORM} <= kinds and ("conv", "q4") in kinds and ("conv", "wide_bf16") in kinds
