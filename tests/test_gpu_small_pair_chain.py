"""GPU tests (``-m gpu``) of the low-resolution backward pairs with a loaded reduction queue: who executes a queued slice must not matter.

The paired launches (small_pair_kernel: convs.hip's data gradient next to a wide weight gradient; conv_wgrad_pair_kernel: the 12-channel
data gradient next to the lean weight gradient) run queued slab reductions at the end of ONE role's blocks -- the conv role where no block
owns more than one item, the weight-gradient role otherwise -- and their walk of the queue (bnerv_side_take with step_over) passes over a
job that is too large for the launch instead of stopping at it.  Each
case here is the smallest shape that reaches its form with ragged tiles, border-only tiles and a partly empty last column tile, B = 2.
Two of the shapes first proposed for the bf16 forms, 30 -> 30 @5x37 and 30 -> 60 s2 @5x18, have rows that are not float4-aligned: every
paired form needs aligned rows, the route query names no pair and the generic weight gradient for them.  They stay in the table with that
answer asserted and run as the two stand-alone launches the caller makes then; their aligned neighbours @5x36 and @5x20 reach the form.

Per case the stream context's queue is loaded, before the pair launch, with
  * a job of 200 slices, more than any of these launches may host (cap = 2 slices per hosting block, at most 48 here): it stays queued;
  * a weight-gradient job (ncols > 0, pushed by a deferred stand-alone weight gradient of a 3 -> 4 channel layer): 4 slices, it fits;
  * a channel-sum job (ncols = 0): 1 slice, it fits -- and sits BEHIND the large one, so it is hosted only if the walk steps over that one.
After the launch exactly two jobs are pending (the large one and the pair's own weight gradient); after one flush every output element is
written (all outputs start as NaN).  dW, db, the per-tile channel sums, dx and the three jobs' outputs are then bit-equal to a second run of
the same descriptors in which the queue was flushed BEFORE the pair launch (the flush kernel executes the jobs, the pair hosts nothing), and
both halves stay within the bounds of tests/test_gpu_conv_families.py against tests/conv_desc_ref.py.  One case per form runs a third time
(loaded queue again) and compares bits with the first."""
import ctypes as C

import pytest
import torch

import conv_family_cases as K
import conv_route_table as T
import test_gpu_conv_families as F
from boosting_nerv_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_COUNT, BIG_SLABS = 6400, 3          # 200 slices of 32 elements
SUM_COUNT, SUM_SLABS = 28, 5            # [B = 2][2][7 channels] from 5 tiles: 1 slice
FIT = dict(kind="wgrad", family=None, B=1, Cin=3, Cout=4, H=9, W=36, k=3, in_mode=L.IN_PLAIN, g_mode=L.IN_PLAIN, g_s=1, db=True, env={})


def _case(name, form, wfam, Cc_in, Cc_out, H, W, c_in, c_ep, in_s, w_in, g_s, aux2=False, twice=False):
    """conv (data gradient): Cc_in -> Cc_out, transposed; weight gradient of the forward layer Cc_out -> Cc_in over the same image."""
    red = c_ep in (L.EP_DSIN, L.EP_DGELU_SAVED)
    env = {"BNERV_SPLIT_WIDE_MIN_TILES": "1"}               # (these images have fewer tiles than the wide families' default floor)
    cv = T.conv_row(Cc_in, Cc_out, H, W, k=3, B=2, in_mode=c_in, ep_mode=c_ep, in_s=in_s, out_s=1, transposed=1, partial=red, env=env)
    wg = dict(B=2, Cin=Cc_out, Cout=Cc_in, H=H, W=W, k=3, in_mode=w_in, g_mode=L.IN_UNSHUFFLE, g_s=g_s)
    return dict(kind="pair", form=form, conv=cv, wgrad=wg, env=env, aux2=aux2, origin="small pair chain", key=None, name=name, wfam=wfam, twice=twice)


CASES = [
    _case("bf16-tat-dgelu-30-9x20", "small_wide", "wide_bf16", 30, 30, 9, 20, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, L.IN_AFFINE, 1, twice=True),
    _case("bf16-tat-dsin-30-9x20", "small_wide", "wide_bf16", 30, 30, 9, 20, L.IN_PLAIN, L.EP_DSIN, 1, L.IN_AFFINE, 1, aux2=True),
    _case("bf16-tat-dgelu-30-5x36", "small_wide", "wide_bf16", 30, 30, 5, 36, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, L.IN_AFFINE, 1),
    _case("bf16-tat-dsin-30-5x36", "small_wide", "wide_bf16", 30, 30, 5, 36, L.IN_PLAIN, L.EP_DSIN, 1, L.IN_AFFINE, 1, aux2=True),
    _case("bf16-up-30to60-5x20", "small_wide", "wide_bf16", 60, 30, 5, 20, L.IN_UNSHUFFLE, L.EP_PLAIN, 2, L.IN_PLAIN, 2, twice=True),
    # rows of 37 and 18 floats are not float4-aligned: the route names no paired form and the generic weight gradient for them (asserted), and
    # the two stand-alone launches the caller then makes go through the same checks
    _case("tat-dgelu-30-5x37", "none", "generic", 30, 30, 5, 37, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, L.IN_AFFINE, 1),
    _case("tat-dsin-30-5x37", "none", "generic", 30, 30, 5, 37, L.IN_PLAIN, L.EP_DSIN, 1, L.IN_AFFINE, 1, aux2=True),
    _case("up-30to60-5x18", "none", "generic", 60, 30, 5, 18, L.IN_UNSHUFFLE, L.EP_PLAIN, 2, L.IN_PLAIN, 2),
    _case("bf16-up-15to48-6x36", "small_wide", "wide_bf16", 48, 15, 6, 36, L.IN_UNSHUFFLE, L.EP_PLAIN, 2, L.IN_PLAIN, 2),
    _case("f32-tat-dgelu-15-6x36", "small_wide", "wide_f32", 15, 15, 6, 36, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, L.IN_AFFINE, 1, twice=True),
    _case("f32-tat-dsin-15-6x36", "small_wide", "wide_f32", 15, 15, 6, 36, L.IN_PLAIN, L.EP_DSIN, 1, L.IN_AFFINE, 1, aux2=True),
    _case("q4-lean-dgelu-12-16x40", "q4_lean", "lean", 12, 12, 16, 40, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, L.IN_AFFINE, 1, twice=True),
    _case("q4-lean-plain-12-16x40", "q4_lean", "lean", 12, 12, 16, 40, L.IN_UNSHUFFLE, L.EP_PLAIN, 1, L.IN_PLAIN, 1),
]


@pytest.fixture(scope="module")
def ops():
    from boosting_nerv_amd import ops as o
    return o


@pytest.fixture(scope="module")
def side_src():
    """The operands of the three preloaded jobs, made once and never written."""
    gen = torch.Generator().manual_seed(20240)
    fit = K.wgrad_operands(dict(FIT, kind="wgrad"), False)
    return dict(big=torch.randn(BIG_SLABS, BIG_COUNT, generator=gen).to(DEV), sums=torch.randn(SUM_SLABS, SUM_COUNT, generator=gen).to(DEV), fit=F._dev(fit))


def _pending():
    return L.load().bnerv_deferred_pending(L.ctx().handle)


def _push_side(ops, src):
    """Queue order: the large job, the weight-gradient job that fits, the channel-sum job."""
    big, sums = F._nan(BIG_COUNT), F._nan(SUM_COUNT)
    n0 = _pending()
    ops._reduce_slabs(src["big"], BIG_SLABS, BIG_COUNT, big, defer=True)
    fit = F._launch_wgrad(ops, FIT, src["fit"], fam_check=False, defer=True)     # (one block: it may host 2 slices, so not the 200 queued before it)
    ops._reduce_slabs(src["sums"], SUM_SLABS, SUM_COUNT, sums, defer=True)
    assert _pending() == n0 + 3, "the three side jobs must all be queued"
    return dict(big=big, sums=sums, fit=fit)


def _run(ops, case, src, preload):
    lib = L.load()
    cv, tc, wg, tw = K.pair_operands(case, False)
    dc = F._dev(tc)
    dwt = {n: (dc["x"] if v is tc["x"] else dc.get("aux0") if v is tc.get("aux0") else dc.get("aux1") if v is tc.get("aux1") else dc.get("scale") if v is tc.get("scale")
               else v.to(DEV).contiguous()) for n, v in tw.items()}
    crun = F._launch_conv(ops, cv, tc, dc, fam_check=False, launch=False)
    wrun = F._launch_wgrad(ops, wg, dwt, fam_check=False, launch=False, defer=True)
    rows = C.c_int(-1)
    form = lib.bnerv_conv_wgrad_pair_form(C.byref(crun["d"]), C.byref(wrun["d"]), C.byref(rows))
    assert (L.PAIR_FORM[form] if form >= 0 else "none") == case["form"], case["name"]
    wfam = L.WGRAD_FAM[lib.bnerv_conv_wgrad_family(C.byref(wrun["d"]), None)]
    assert wfam == case["wfam"], (case["name"], wfam)
    ops._flush_deferred()
    assert _pending() == 0
    side = _push_side(ops, src)
    if not preload:
        ops._flush_deferred()                               # the flush kernel executes the three jobs; the pair finds an empty queue
    if case["form"] == "none":                              # what ops._wgrad_conv_pair does when the library takes no pair
        L.check(lib.bnerv_conv_wgrad(L.stream(), C.byref(wrun["d"])), "bnerv_conv_wgrad")
        L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(crun["d"])), "bnerv_conv_igemm")
        assert _pending() >= 1
    else:
        assert lib.bnerv_conv_wgrad_pair(L.stream(), C.byref(crun["d"]), C.byref(wrun["d"])) == 0, lib.bnerv_last_error()
        # loaded queue: the two small jobs were hosted although the large one is in front of them; it and the pair's own weight gradient wait
        assert _pending() == (2 if preload else 1), (case["name"], preload, _pending())
    ops._flush_deferred()
    torch.cuda.synchronize()
    got = dict(dx=crun["out"], dw=wrun["dw"], db=wrun["db"], big=side["big"], sums=side["sums"], fit_dw=side["fit"]["dw"], fit_db=side["fit"]["db"])
    if crun["part"] is not None:
        got["part"] = crun["part"][:crun["rows"]]
    for n, v in got.items():
        assert torch.isfinite(v).all(), f"{case['name']} (preload={preload}): {n} has elements that were never written"
    return dict(got=got, crun=crun, wrun=wrun, wfam=wfam, ops_in=(cv, tc, wg, tw), keep=side)


def _same_bits(tag, a, b):
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{tag}: {n} differs in {(a[n] != b[n]).sum().item()} of {a[n].numel()} elements"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_hosted_jobs_change_no_bit(ops, side_src, case, monkeypatch):
    F._env(monkeypatch, case["env"])
    assert K.pair_form(case)[0] == case["form"], "the host route query on made-up pointers names another form"
    loaded = _run(ops, case, side_src, preload=True)
    empty = _run(ops, case, side_src, preload=False)
    _same_bits(case["name"] + " loaded queue vs flushed queue", loaded["got"], empty["got"])
    if case["twice"]:
        again = _run(ops, case, side_src, preload=True)
        _same_bits(case["name"] + " second run", loaded["got"], again["got"])
    cv, tc, wg, tw = loaded["ops_in"]
    split = loaded["wfam"] in K.SPLIT_WGRAD
    F._check_conv(ops, cv, tc, K.reference(cv, tc), loaded["crun"], False, split=False, fam="pair/" + case["form"])
    F._check_wgrad(wg, tw, K.reference(wg, tw), loaded["wrun"], False, split=split, fam="pair/" + case["form"], tag=case["name"] + " weight half")
    fit_t = {n: v.cpu() for n, v in side_src["fit"].items()}
    F._check_wgrad(FIT, fit_t, K.reference(FIT, fit_t), loaded["keep"]["fit"], False, split=False, fam="hosted", tag=case["name"] + " hosted weight gradient")
    for name, srcn in (("big", "big"), ("sums", "sums")):
        ref = side_src[srcn].double().sum(0).cpu()
        n_slabs = side_src[srcn].shape[0]
        allow = (n_slabs + 2) * K.U * side_src[srcn].double().abs().sum(0).cpu()
        F._within(f"{case['name']} hosted {name}", loaded["got"][name], ref, allow, fam="hosted")
