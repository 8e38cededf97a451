"""CPU tests of the case table of the per-family numerical tests (tests/conv_family_cases.py; the GPU half is
tests/test_gpu_conv_families.py): every case reaches the family it is about, the table covers every instantiation a shipped
configuration launches, the exact-pass operands are ones on which equality with float64 is owed, and the exact comparison flags a
single missing product at exactly its output element.  Made-up pointers: nothing is launched."""
import pytest
import torch

import conv_desc_ref as R
import conv_family_cases as K
from boosting_nerv_amd import _lib as L


def _representable(name, x, case):
    assert bool((x.float().double() == x).all()), f"{K.case_id(case)}: {name} is not exactly representable in f32"


def test_every_shipped_key_and_every_mode_found_a_shape():
    b = K.build()
    assert not b["missing"], b["missing"]
    ids = [K.case_id(c) for kind in ("conv", "wgrad", "pair", "conv5") for c in b[kind]]
    assert len(ids) == len(set(ids))


def test_every_case_runs_on_the_family_it_is_about():
    b = K.build()
    for c in b["conv"]:
        fam, rows, _ = K.conv_family(c)
        assert fam == c["family"], (K.case_id(c), fam)
        th, tw = K.tile_of(fam)
        assert rows == -(-c["H"] // th) * -(-c["W"] // tw), (K.case_id(c), rows)
        assert c["H"] * c["W"] <= 70000
    lib = L.load()
    for c in b["wgrad"]:                    # family, and the slabs it writes: none for the stem kernel, otherwise inside the mode-free workspace
        fam, n_slabs = K.wgrad_family(c)
        assert fam == c["family"], K.case_id(c)
        ws = lib.bnerv_conv_wgrad_ws_bytes(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["k"])
        assert (n_slabs == 0) == (fam == "stem") and 0 <= n_slabs * c["Cout"] * (c["Cin"] * c["k"] ** 2 + 1) * 4 <= ws, (K.case_id(c), n_slabs, ws)
    for c in b["pair"]:
        form, rows = K.pair_form(c)
        assert form == c["form"], (K.case_id(c), form)
        if c["conv"]["ep_mode"] in R.SUMS_EP:
            assert rows == K.conv_family(c["conv"])[1] > 0, K.case_id(c)


def test_every_family_mode_pair_has_a_case():
    have = {(c["family"], L.IN_PLAIN if (c["in_mode"] == L.IN_UNSHUFFLE and c["in_s"] == 1) else c["in_mode"], c["ep_mode"], c["out_s"]) for c in K.build()["conv"]}
    lacking = [(fam, m) for fam, table in K.MODE_TABLES.items() for m in table if (fam,) + m not in have]
    assert not lacking, lacking


@pytest.mark.parametrize("config", ["c1", "c3", "c4", "hnerv"])
def test_the_table_covers_every_shipped_instantiation(config):
    b = K.build()
    pinned = K.pinned_keys(config)
    have = {"conv": {c["key"] for c in b["conv"]}, "wgrad": {c["key"] for c in b["wgrad"]}, "pair": {c["key"] for c in b["pair"]}}
    uncovered = [(kind, key) for kind in ("conv", "wgrad", "pair") for key in pinned[kind] if key[0] != "none" and key not in have[kind]]
    for u in uncovered:
        print("uncovered:", config, u)
    assert not uncovered, uncovered
    for key in pinned["pair"]:              # a declined pair is two stand-alone calls: both halves have a case of their own
        if key[0] == "none":
            _, im, ep, k, in_s, wim, gm, gs = key
            assert any(c["key"][1:6] == (im, ep, k, in_s, 1) for c in b["conv"]), key
            assert any(c["key"][1:5] == (k, wim, gm, gs) for c in b["wgrad"]), key


def test_edge_conditions_per_shipped_key():
    """_find relaxes the edge conditions silently where no candidate meets them all, so what every case met is asserted here.  Every
    shipped conv / weight-gradient key has a case with H, W off the tile, ragged Cout, B = 2 -- and ragged Cin wherever a layer of its family
    can have it (the PixelShuffle(2) gradients gather multiples of 4, the 1x1 head has 12 inputs).  The pairs: the same, where Cout is the
    conv half's (the weight half's Cin) -- except that the 1x1 head's data gradient has 12 outputs, and the wide pair gathers through
    PixelShuffle(2).  The stem kernel takes at most 256 pixels: one of its two cases is ragged in H, the other in W (both at once do not fit)."""
    b = K.build()
    for c in b["conv"] + b["wgrad"]:
        if c["origin"] != "shipped":
            continue
        need = {"B", "H", "W", "Cout"} | ({"Cin"} if c.get("in_s", 1) != 2 and c["family"] != "head1_fwd" else set())
        assert need <= set(c["edges"]), (K.case_id(c), c["edges"])
    for c in b["pair"]:
        v = c["conv"]
        need = {"B", "H", "W"} | ({"Cout"} if c["form"] != "head" else set()) | ({"Cin"} if v["in_s"] != 2 else set())
        if c["form"] == "stem":             # (<= 256 pixels, 4x16 tiles: ragged in both directions at 5x20)
            assert (v["H"], v["W"]) == (5, 20)
        assert need <= set(c["edges"]), (K.case_id(c), c["edges"])
    stem = [c for c in b["conv"] if c["family"] == "stem_dgrad"]
    assert len(stem) == 2 and all({"B", "Cin", "Cout"} <= set(c["edges"]) for c in stem)
    assert {"H", "W"} <= set(stem[0]["edges"]) | set(stem[1]["edges"]), [c["edges"] for c in stem]
    for c in b["conv"]:                     # the mode-table cases and the NULL variants inherit or meet the full set
        if c["family"] != "stem_dgrad" and c["origin"] != "stem slabs, partial flipped":
            assert {"B", "H", "W", "Cout"} <= set(c["edges"]), (K.case_id(c), c["edges"])


def _check_conv_operands(c, t):
    r = K.reference(c, t)
    if not K.pre_exact(c):
        return
    m = r["mid"]
    q = R.quantum(r["a"]) * R.quantum(r["weff"])
    for n in ("a", "v", "u"):
        if n in m:
            _representable(n, m[n], c)
    bound = R.abs_bound(c["kind"], c, t).max().item()
    assert bound < 2.0 ** 24 * q, (K.case_id(c), bound, q)
    if K.out_exact(c):
        for n in ("vs", "t", "v_aux", "out_conv_space"):
            if n in m:
                _representable(n, m[n], c)
        if r["sums"] is not None:
            _representable("(ds, dt)", r["sums"], c)
            assert m["sum_abs"].max().item() < 2.0 ** 24 * R.quantum(m["v_aux"], r["v"]), K.case_id(c)


def _check_wgrad_operands(c, t):
    if not K.pre_exact(c):
        return
    r = K.reference(c, t)
    ab = R.abs_bound(c["kind"], c, t)
    qa, qg = R.quantum(r["a"]), R.quantum(r["g"])
    for n in ("a", "g", "dw", "db"):
        _representable(n, r[n], c)
    assert ab["dw"].max().item() < 2.0 ** 24 * qa * qg and ab["db"].max().item() < 2.0 ** 24 * qg, K.case_id(c)


def test_exact_pass_operands_are_ones_on_which_equality_is_owed():
    """On the exact pass's operands the float64 result and every intermediate of the header's formulas are f32 numbers, and sum |a| |b|
    stays below 2^24 quanta: then every partial sum, in any order, with or without split-K or slabs, is exact in f32."""
    b = K.build()
    for c in b["conv"] + [c for c in b["conv5"] if c["kind"] == "conv5"]:
        _check_conv_operands(c, K.conv_operands(c, True))
    for c in b["wgrad"] + [c for c in b["conv5"] if c["kind"] == "conv5_wgrad"]:
        _check_wgrad_operands(c, K.wgrad_operands(c, True))
    for c in b["pair"]:
        cv, tc, wg, tw = K.pair_operands(c, True)
        _check_conv_operands(cv, tc)
        _check_wgrad_operands(wg, tw)


def _pick(cases, pred):
    return next(c for c in cases if pred(c))


def _smallest_term_conv(r, b, co, y, x, ci, k):
    """(value, tap) of the smallest non-zero product a[b][ci][y+ty-p][x+tx-p] * W[co][ci][ty][tx] of output element (b, co, y, x)."""
    p, best = (k - 1) // 2, None
    H, W = r["a"].shape[2:]
    for ty in range(k):
        for tx in range(k):
            yy, xx = y + ty - p, x + tx - p
            if 0 <= yy < H and 0 <= xx < W:
                term = (r["a"][b, ci, yy, xx] * r["weff"][co, ci, ty, tx]).item()
                if term != 0 and (best is None or abs(term) < abs(best)):
                    best = term
    return best


@pytest.mark.parametrize("which", ["long-K data gradient", "sums epilogue", "weight gradient"])
def test_exact_comparison_flags_one_missing_product(which):
    """Comparator self-test: the float64 result cast to f32 stands in for a kernel that is right; the reference loses the single smallest
    non-zero product at a corner pixel of the last input channel (the last pixel, for the weight gradient).  `==` reports exactly that
    element.  The random pass's allowance at that element is printed beside the removed term."""
    b = K.build()
    if which == "weight gradient":
        c = _pick(b["wgrad"], lambda c: c["family"] == "wide_f32" and c["in_mode"] == L.IN_AFFINE)
        t = K.wgrad_operands(c, True)
        r = K.reference(c, t)
        kernel = r["dw"].float()
        co, ci, bb, y, x = c["Cout"] - 1, c["Cin"] - 1, c["B"] - 1, c["H"] - 1, c["W"] - 1
        term = (r["g"][bb, co, y, x] * r["a"][bb, ci, y, x]).item()                     # the centre tap reads the last pixel itself
        if term == 0:
            co = next(o for o in range(c["Cout"]) if r["g"][bb, o, y, x] != 0)
            term = (r["g"][bb, co, y, x] * r["a"][bb, ci, y, x]).item()
        assert term != 0
        broken = r["dw"].clone()
        broken[co, ci, 1, 1] -= term
        bad = (kernel != broken.float()).nonzero().tolist()
        assert bad == [[co, ci, 1, 1]], bad
        rnd = K.wgrad_operands(c, False)
        allow = K.wgrad_allowance(c, rnd, split=True)["dw"][co, ci, 1, 1].item()
        print(f"{K.case_id(c)}: removed term {term:g} of dw[{co},{ci},1,1]; random-pass allowance there {allow:.3g} (ratio {abs(term) / allow:.3g})")
        return
    if which == "long-K data gradient":
        c = _pick(b["conv"], lambda c: c["transposed"] and c["in_s"] == 5 and c["partial"])
    else:
        c = _pick(b["conv"], lambda c: c["family"] == "small96" and c["ep_mode"] == L.EP_DSIN and c["aux2"])
    t = K.conv_operands(c, True)
    r = K.reference(c, t)
    bb, ci = c["B"] - 1, c["Cin"] - 1                                                   # a corner pixel (the first with a non-zero product), the last channel
    nz = lambda n, o, y, x: t.get(n) is None or t[n][bb, o, y, x].item() != 0          # (a zero gate or multiplier would hide the term: the case is deterministic, so pick past it)
    y, x, co = next((y, x, o) for y in (c["H"] - 1, 0) for x in (c["W"] - 1, 0) for o in reversed(range(c["Cout"]))
                    if _smallest_term_conv(r, bb, o, y, x, ci, c["k"]) is not None and nz("aux2", o, y, x) and (which != "sums epilogue" or nz("aux0", o, y, x)))
    term = _smallest_term_conv(r, bb, co, y, x, ci, c["k"])
    delta = torch.zeros_like(r["v"])
    delta[bb, co, y, x] = -term
    broken = K.reference(c, t, v_delta=delta)
    bad = (r["out"].float() != broken["out"].float()).nonzero().tolist()
    assert bad == [[bb, co, y, x]], bad
    if which == "sums epilogue":
        bad_s = (r["sums"].float() != broken["sums"].float()).nonzero().tolist()
        assert bad_s == [[bb, 0, co], [bb, 1, co]], bad_s
    rnd = K.conv_operands(c, False)
    allow = K.conv_allowance(c, rnd, K.reference(c, rnd), split=False)
    a_out = allow["out"][bb, co, y, x].item()
    print(f"{K.case_id(c)}: removed term {term:g} of v[{bb},{co},{y},{x}] (K = {c['Cin'] * c['k'] ** 2}); random-pass allowance there {a_out:.3g} "
          f"(ratio {abs(term) / a_out:.3g})" + (f", on dt {allow['sums'][bb, 1, co].item():.3g}" if allow["sums"] is not None else ""))
