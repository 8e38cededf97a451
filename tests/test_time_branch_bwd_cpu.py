"""CPU suite (``-m "not gpu"``): the host side of bnerv_time_branch_bwd (include/bnerv.h; the time-embedding branch's backward as two
launches).  Everything the entry point decides, it decides before its first device call, so its argument validation, its "not my shapes"
answer and the layout of its by-value tables can be checked on a machine without a GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _desc(L, B=1, Lv=80, SH=256, SO=4320, TH=64, TO=32, n_mlp=32, widths=None, keep=None):
    """A descriptor whose pointers are non-null host addresses: the calls below must return before anything dereferences them."""
    buf = (C.c_float * 16)()
    keep.append(buf)
    p = C.addressof(buf)
    d = L.TimeBranchBwdDesc()
    for name, _ in L.TimeBranchBwdDesc._fields_:
        if name not in ("B", "L", "SH", "SO", "TH", "TO", "n_mlp", "_pad", "d_ty1"):
            setattr(d, name, p)
    d.B, d.L, d.SH, d.SO, d.TH, d.TO, d.n_mlp = B, Lv, SH, SO, TH, TO, n_mlp
    widths = widths if widths is not None else [12] * max(n_mlp, 1)
    ml = (L.TimeBranchBwdMlp * max(len(widths), 1))()
    for i, c in enumerate(widths):
        for name in ("w1", "w2", "hs", "d_out", "dw1", "db1", "dw2", "db2"):
            setattr(ml[i], name, p)
        ml[i].C = c
    return d, ml


def test_time_branch_bwd_rejects_bad_arguments_with_a_message():
    from boosting_nerv_amd import _lib as L
    lib, keep = L.load(), []
    d, ml = _desc(L, keep=keep)
    assert lib.bnerv_time_branch_bwd(None, None, ml) == -1
    assert b"null descriptor" in lib.bnerv_last_error()
    assert lib.bnerv_time_branch_bwd(None, C.byref(d), None) == -1
    assert b"null descriptor" in lib.bnerv_last_error()
    for n in (0, -3):
        d, ml = _desc(L, n_mlp=n, keep=keep)
        assert lib.bnerv_time_branch_bwd(None, C.byref(d), ml) == -1
        assert b"at least one modulation MLP" in lib.bnerv_last_error()
    d, ml = _desc(L, keep=keep)
    d.d_sw1 = None
    assert lib.bnerv_time_branch_bwd(None, C.byref(d), ml) == -1
    assert b"null gradient output" in lib.bnerv_last_error()
    d, ml = _desc(L, keep=keep)
    ml[5].hs = None
    assert lib.bnerv_time_branch_bwd(None, C.byref(d), ml) == -1
    assert b"bad modulation MLP 5" in lib.bnerv_last_error()


@pytest.mark.parametrize("over", [dict(B=5), dict(Lv=129), dict(SH=4097), dict(TH=65), dict(TO=33), dict(n_mlp=40, widths=[12] * 40),
                                  dict(n_mlp=3, widths=[12, 129, 12])])
def test_time_branch_bwd_declines_over_limit_shapes_before_any_device_call(over):
    """Same limits as the forward (B <= 4, 2L <= 256, SH <= 4096, TH <= 64, TO <= 32, C_i <= 128) and n_mlp + 1 groups of the grouped
    table: 1 = "run the five grouped launches".  The pointers are host addresses and there is no device here: a launch, or a read of any
    tensor, would fail or fault instead of returning 1."""
    from boosting_nerv_amd import _lib as L
    lib, keep = L.load(), []
    d, ml = _desc(L, keep=keep, **over)
    assert lib.bnerv_time_branch_bwd(None, C.byref(d), ml) == 1


def test_time_branch_bwd_tables_have_the_header_layout_and_fit_the_argument_segment():
    from boosting_nerv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    mlp_bytes = int(re.search(r"#define BNERV_TIME_BRANCH_BWD_MLP_BYTES (\d+)", header).group(1))
    desc_bytes = int(re.search(r"#define BNERV_TIME_BRANCH_BWD_DESC_BYTES (\d+)", header).group(1))
    assert C.sizeof(L.TimeBranchBwdMlp) == mlp_bytes == L.TIME_BRANCH_BWD_MLP_BYTES
    assert C.sizeof(L.TimeBranchBwdDesc) == desc_bytes == L.TIME_BRANCH_BWD_DESC_BYTES
    # field for field (names and order) against the header's typedefs
    for struct, cname in ((L.TimeBranchBwdMlp, "bnerv_time_branch_bwd_mlp"), (L.TimeBranchBwdDesc, "bnerv_time_branch_bwd_desc")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|int)\s*\*?", "", decl).split(",")]
        assert names == [n for n, _ in struct._fields_], cname
    # launch A carries the stem's layer 1 as one grouped descriptor (+ B), an entry per MLP -- at most MAX_DENSE_GROUPS - 1 = 39, the
    # five-launch form's own limit -- two pointers and six ints, all by value in the <= 4096-byte kernel-argument segment
    n_max = L.MAX_DENSE_GROUPS - 1
    assert n_max == 39
    assert C.sizeof(L.DenseBwdDesc) + 8 + n_max * C.sizeof(L.TimeBranchBwdMlp) + 2 * 8 + 6 * 4 <= 4096
