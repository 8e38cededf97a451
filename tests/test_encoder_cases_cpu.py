"""CPU checks of tests/encoder_cases.py, the case tables and bounds that tests/test_gpu_encoder_ops.py runs on the GPU:
every row hits the launch plan it claims (asked of the library's two host-only plan queries), the tables cover every cnx_mlp
instantiation, the float32 stock-op computation of each operator stays inside the bounds and tolerances against float64, each of a set
of one-element / one-tile mutations of that computation is rejected, and the entry points refuse what they are not built for before
any launch."""
import ctypes as C

import pytest
import torch

import encoder_cases as E
from boosting_nerv_amd import _lib as L
from test_alignment_cpu import _p, _refused

cid = lambda c: c.id


# ------------------------------------------------------------------------------------------------------------ plans and coverage
@pytest.mark.parametrize("c", E.CNX_CASES, ids=cid)
def test_cnx_row_hits_the_plan_it_claims(c):
    HW = c.H * c.W
    nt, grid, items = E.mlp_plan(c.B, c.C, HW)
    assert nt == c.nt, (c, nt)
    assert items == c.B * -(-HW // (16 * nt)) and 1 <= grid <= -(-items // 4)
    assert (grid * 4 < items) == c.trip, (c, grid, items)
    assert grid <= (256 if c.C == 64 else 512)


def test_cnx_rows_hit_the_tile_edges_by_name():
    by = {c.id: c for c in E.CNX_CASES}
    assert E.mlp_plan(1, 16, 16384)[0] == 1 and E.mlp_plan(1, 16, 16385)[0] == 2            # the threshold itself, either side
    assert by["thr-C16-1x128x128"].H * by["thr-C16-1x128x128"].W == 16384
    tails = sorted({(c.H * c.W) % 32 for c in E.CNX_CASES if c.id.startswith("nt2-")})
    assert tails == [0, 7, 16, 23]
    for C_ in E.CNX_DIMS:
        assert {(c.H * c.W) % 32 for c in E.CNX_CASES if c.id.startswith("nt2-") and c.C == C_} >= {7}
        assert any(c.C == C_ and c.H * c.W < 16 for c in E.CNX_CASES)
        assert any(c.C == C_ and c.B > 1 and (c.H * c.W) % 16 and c.nt == 1 for c in E.CNX_CASES)
        assert any(c.C == C_ and c.B > 1 and 1 <= (c.H * c.W) % 32 <= 16 and c.nt == 2 for c in E.CNX_CASES)     # second half-tile dead
        assert any(c.C == C_ and c.w1s == 30.0 for c in E.CNX_CASES)
    for C_ in (16, 64):
        assert {(c.H * c.W) % 32 for c in E.CNX_CASES if c.id.startswith("nt2-") and c.C == C_} == {0, 7, 16, 23}
    assert by["trip2-C64-1x150x221"] and E.mlp_plan(1, 64, 150 * 221)[1:] == (256, 1036)
    assert E.mlp_plan(1, 48, 257 * 256)[1:] == (512, 2056) and E.mlp_plan(100, 64, 7 * 23) == (1, 256, 1100)
    assert {c.nt for c in E.CNX_CASES if not c.gamma} == {1, 2}


def test_cnx_rows_cover_every_instantiation_and_a_second_trip_for_both_tile_counts():
    assert {(c.C, c.nt) for c in E.CNX_CASES} == {(C_, nt) for C_ in E.CNX_DIMS for nt in (1, 2)}
    assert {c.nt for c in E.CNX_CASES if c.trip} == {1, 2}
    assert len({c.id for c in E.CNX_CASES}) == len(E.CNX_CASES)


@pytest.mark.parametrize("c", E.DW_CASES, ids=cid)
def test_dwconv_row_hits_the_plan_it_claims(c):
    groups, rows = E.dw_plan(c.B, c.C, c.H, c.W)
    tiles_y = -(-c.H // E.DW_TILE_H)
    assert 1 <= groups <= tiles_y and rows == -(-tiles_y // groups) and (groups - 1) * rows < tiles_y     # no empty group
    if c.groups is not None:
        assert (groups, rows) == (c.groups, c.rows), (c, groups, rows)


def test_dwconv_rows_hit_the_edges_by_name():
    by = {(c.B, c.C, c.H, c.W, c.K): c for c in E.DW_CASES}
    assert tiles_left(by[(8, 64, 80, 20, 7)]) == 2 and tiles_left(by[(16, 64, 40, 20, 3)]) == 3
    assert {c.W - E.dw_last_tile_column(c.W) for c in E.DW_CASES if c.W > 64} >= {1, 2, 3, 4}
    assert any(c.K == 1 for c in E.DW_CASES) and any(c.H < c.K and c.W < c.K and c.H * c.W > 1 for c in E.DW_CASES)
    assert any(c.W % 4 == 0 and c.W > 64 for c in E.DW_CASES) and any(c.W % 4 and c.W > 64 for c in E.DW_CASES)
    assert {c.K for c in E.DW_CASES} == {1, 3, 5, 7}


def tiles_left(c):
    """Tile rows in the last group of the weight-gradient launch."""
    groups, rows = E.dw_plan(c.B, c.C, c.H, c.W)
    return -(-c.H // E.DW_TILE_H) - (groups - 1) * rows


def test_layernorm_rows_cover_every_width_and_length():
    assert {c.C for c in E.LN_CASES} == set(E.LN_C) and {c.HW for c in E.LN_CASES} == set(E.LN_HW) and {c.B for c in E.LN_CASES} == {1, 3}
    assert 13 <= len(E.LN_CASES) <= 18
    # the backward gives wave q channels [q CQ, (q + 1) CQ), CQ = (C + 3) >> 2: rows with an idle wave and with a short one
    short = lambda c: [max(0, min(c, (q + 1) * ((c + 3) >> 2)) - q * ((c + 3) >> 2)) for q in range(4)]
    assert any(0 in short(c.C) for c in E.LN_CASES) and any(0 < short(c.C)[3] < short(c.C)[0] for c in E.LN_CASES)


def test_patchify_rows_sit_where_they_claim():
    lib = L.load()
    for c in E.PATCH_CASES:
        rows, K = c.B * (c.H // c.s) * (c.W // c.s), c.Cin * c.s * c.s
        assert (lib.bnerv_dense_gemm_bwd_ws_bytes(rows, K, c.Cout) > 0) == c.split, c
    a, b, _ = E.PATCH_CASES
    assert a.split and a.H % a.s and a.W % a.s and a.B * (a.H // a.s) * (a.W // a.s) == 4608
    assert not b.split and b.Cin * b.s * b.s == 576 and b.B * (b.H // b.s) * (b.W // b.s) == 252 and b.H % b.s and b.W % b.s
    assert [lib.bnerv_dense_gemm_bwd_ws_bytes(r, i, o) > 0 for r, i, o in E.GEMM_CASES] == [False, True, True]
    assert [r for r, _, _ in E.GEMM_CASES] == [E.GEMM_SPLIT_ROWS - 1, E.GEMM_SPLIT_ROWS, E.GEMM_SPLIT_ROWS + 1]


def test_plan_queries_answer_on_the_host_and_refuse_what_is_not_built():
    lib = L.load()
    nt = C.c_int(-7)
    _refused(lib.bnerv_cnx_mlp_plan(1, 24, 64, C.byref(nt), None, None), "cnx_mlp", "C must be 16, 32, 48 or 64")
    assert nt.value == -7
    _refused(lib.bnerv_cnx_mlp_plan(0, 16, 64, None, None, None), "cnx_mlp_plan")
    _refused(lib.bnerv_dwconv_wgrad_plan(1, 1, 0, 5, None, None), "dwconv_wgrad_plan")
    assert lib.bnerv_cnx_mlp_plan(1, 16, 64, None, None, None) == 0 and lib.bnerv_dwconv_wgrad_plan(1, 1, 5, 5, None, None) == 0
    # c3's first encoder stage, 216 x 384 at C = 64: NT = 2 on the capped grid; depthwise weight gradient in 3 groups of 5 tile rows (last: 4)
    assert E.mlp_plan(1, 64, 216 * 384) == (2, 256, 2592) and E.dw_plan(1, 64, 216, 384) == (3, 5)


# ------------------------------------------------------------------------------------------------------------ bounds and mutations
def _ok(check, got, ref):
    return E.passes(*check(got, ref))


def _failed(check, got, ref, names):
    """Every name in `names` is rejected (a ratio above 1 or a failed close())."""
    ratios, oks = check(got, ref)
    return [n for n in names if (ratios[n] <= 1.0 if n in ratios else oks[n])] == []


def test_cnx_reference_is_the_gradient_of_the_stock_expression():
    """The written-out float64 backward of cnx_reference against float64 autograd over cnx_ref, with and without gamma."""
    for c in (E.CNX_CASES[4], next(c for c in E.CNX_CASES if not c.gamma)):
        d = E.cnx_inputs(c)
        ref, auto = E.cnx_reference(d), E.cnx_stock(d, torch.float64)
        for n in ("out", "dx", "dinp") + E.CNX_SUMMED:
            if ref[n] is None:
                assert auto[n] is None
            else:
                assert float((ref[n] - auto[n]).abs().max()) <= 1e-12 * (1 + float(ref[n].abs().max())), n


@pytest.mark.parametrize("c", [c for c in E.CNX_CASES if not c.trip], ids=cid)
def test_cnx_float32_stays_inside_the_bounds_and_mutations_do_not(c):
    d = E.cnx_inputs(c)
    ref = E.cnx_reference(d)
    ratios, oks = E.check_cnx(E.cnx_stock(d), ref)
    assert E.passes(ratios, oks), (ratios, oks)
    assert max(ratios.values()) < 0.25, ratios              # float32 on stock ops is nowhere near the bound: the bound is no fit to it
    summed = [n for n in E.CNX_SUMMED if ref[n] is not None]
    assert _failed(E.check_cnx, E.cnx_stock(d, drop_hidden=4 * c.C - 3), ref, ["out", "dx"])
    assert _failed(E.check_cnx, E.cnx_stock(d, lose_tail=16), ref, ["out", "dx"] + summed)


@pytest.mark.parametrize("c", E.DW_CASES, ids=cid)
def test_dwconv_float32_stays_inside_the_bounds_and_mutations_do_not(c):
    d = E.dw_inputs(c)
    ref = E.dw_reference(d)
    ratios, oks = E.check_dw(E.dw_stock(d), ref)
    assert E.passes(ratios, oks), (ratios, oks)
    assert _failed(E.check_dw, E.dw_stock(d, drop_tap=True), ref, ["y", "dx"])
    assert _failed(E.check_dw, E.dw_stock(d, shift=True), ref, ["y", "dx"])
    assert _failed(E.check_dw, E.dw_stock(d, lose_tile=True), ref, ["dw", "db"])


@pytest.mark.parametrize("c", E.LN_CASES, ids=cid)
def test_layernorm_float32_stays_inside_the_tolerance_and_mutations_do_not(c):
    d = E.ln_inputs(c)
    ref = E.ln_reference(d)
    ratios, oks = E.check_ln(E.ln_stock(d), ref)
    assert E.passes(ratios, oks), oks
    assert _failed(E.check_ln, E.ln_stock(d, leave_out=1), ref, ["y"])
    # (one channel is its own mean: xhat = 0 and dw = 0 whatever is summed)
    assert _failed(E.check_ln, E.ln_stock(d, lose_block=True), ref, ["dw", "db"] if c.C > 1 else ["db"])


@pytest.mark.parametrize("c", E.PATCH_CASES, ids=cid)
def test_patchify_float32_stays_inside_the_bounds_and_mutations_do_not(c):
    d = E.patch_inputs(c)
    ref = E.patch_reference(d)
    ratios, oks = E.check_patch(E.patch_stock(d), ref)
    assert E.passes(ratios, oks), (ratios, oks)
    Hc, Wc = (c.H // c.s) * c.s, (c.W // c.s) * c.s
    assert float(ref["e_dx"][:, :, Hc:].abs().sum()) == 0 and float(ref["e_dx"][:, :, :, Wc:].abs().sum()) == 0      # exact zeros asked there
    assert float(ref["e_dx"][:, :, :Hc, :Wc].min()) > 0
    assert _failed(E.check_patch, E.patch_stock(d, drop_weight=True), ref, ["y", "dx"])
    assert _failed(E.check_patch, E.patch_stock(d, lose_rows=16), ref, ["dw", "db"])


@pytest.mark.parametrize("rows,I,O", E.GEMM_CASES)
def test_dense_gemm_float32_stays_inside_the_bounds_and_mutations_do_not(rows, I, O):
    d = E.gemm_inputs(rows, I, O)
    ref = E.gemm_reference(d)
    ratios, oks = E.check_patch(E.gemm_stock(d), ref)
    assert E.passes(ratios, oks), (ratios, oks)
    assert _failed(E.check_patch, E.gemm_stock(d, drop_weight=True), ref, ["y", "dx"])
    assert _failed(E.check_patch, E.gemm_stock(d, lose_rows=16), ref, ["dw", "db"])


def test_bound_ratio_asks_for_exact_values_where_the_bound_is_zero():
    ref, bound = torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 1e-6, 0.0], dtype=torch.float64)
    assert E.bound_ratio(torch.tensor([0.0, 5e-7, 0.0]), ref, bound) == pytest.approx(0.5, rel=1e-3)
    assert E.bound_ratio(torch.tensor([0.0, 0.0, 1e-30]), ref, bound) == float("inf")
    assert E.bound_ratio(torch.tensor([0.0, float("nan"), 0.0]), ref, bound) == float("inf")
    assert not E.close_ok(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64), "y fwd")


# ------------------------------------------------------------------------------------------------------------ refusals
def test_cnx_mlp_refuses_a_width_it_is_not_built_for_before_any_launch():
    lib = L.load()
    rc = lib.bnerv_cnx_mlp_fwd(None, _p(0), _p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), None, 1, 24, 64)
    _refused(rc, "cnx_mlp", "C must be 16, 32, 48 or 64", "24")
    rc = lib.bnerv_cnx_mlp_bwd(None, _p(0), _p(1), _p(2), _p(4), _p(6), _p(7), _p(8), _p(9), 1, 24, 64)
    _refused(rc, "cnx_mlp", "C must be 16, 32, 48 or 64", "24")


@pytest.mark.parametrize("B,Cc,word", [(1, 0, "C must be in [1, 64]"), (1, 65, "C must be in [1, 64]"), (65536, 16, "B too large")])
def test_layernorm_refuses_before_any_launch(B, Cc, word):
    lib = L.load()
    _refused(lib.bnerv_lncf_fwd(None, _p(0), _p(1), _p(2), _p(3), B, Cc, 64, 1e-6), "lncf_fwd", word)
    _refused(lib.bnerv_lncf_bwd(None, _p(0), _p(1), _p(2), _p(3), _p(4), _p(5), 1 << 40, B, Cc, 64, 1e-6), "lncf_bwd", word)


@pytest.mark.parametrize("B,Cc,K,word", [(1, 4, 2, "K must be odd"), (1, 4, 9, "K must be odd"), (1024, 64, 7, "B*C too large")])
def test_dwconv_refuses_before_any_launch(B, Cc, K, word):
    lib = L.load()
    _refused(lib.bnerv_dwconv_fwd(None, _p(0), _p(1), _p(2), _p(3), B, Cc, 8, 8, K, 0), "dwconv_fwd", word)
    _refused(lib.bnerv_dwconv_wgrad(None, _p(0), _p(1), _p(2), _p(3), 1 << 40, B, Cc, 8, 8, K, None), "dwconv_wgrad", word)
