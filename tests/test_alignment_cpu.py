"""CPU tests of the pointer-alignment contract (INTEGRATION.md "Pointer alignment"): the entry points validate before they touch the
device (as test_host_cpu.test_abi_argument_validation_without_gpu relies on), so refusals and alignment-dependent workspace sizes can be
checked with made-up pointer values; ops.time_branch decides on the host."""
import ctypes as C

import pytest
import torch

from boosting_nerv_amd import _lib as L

BASE = 0x7F0000000000        # a made-up, 16-byte aligned "device" address; nothing is dereferenced before the checks under test


def _p(i, off=0):
    return C.c_void_p(BASE + 0x100000 * i + off)


def _refused(rc, *words):
    msg = L.load().bnerv_last_error().decode()
    assert rc == -1, (rc, msg)                              # BNERV_E_ARG
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("off", [4, 8, 12])
def test_cnx_mlp_refuses_misaligned_weights_and_names_them(off):
    lib = L.load()
    for w1, w2 in ((off, 0), (0, off)):
        rc = lib.bnerv_cnx_mlp_fwd(None, _p(0), _p(1), _p(2, w1), _p(3), _p(4, w2), _p(5), _p(6), _p(7), None, 1, 16, 64)
        _refused(rc, "cnx_mlp_fwd", "w1", "w2", "16-byte aligned")
        rc = lib.bnerv_cnx_mlp_bwd(None, _p(0), _p(1), _p(2, w1), _p(4, w2), _p(6), _p(7), _p(8), _p(9), 1, 16, 64)
        _refused(rc, "cnx_mlp_bwd", "w1", "w2", "16-byte aligned")


def test_fetch_frame_refuses_misaligned_frames_and_names_them():
    lib = L.load()
    _refused(lib.bnerv_fetch_frame(None, _p(0, 4), None, _p(1), 3, 64, _p(2), None), "fetch_frame", "clip", "16-byte aligned")
    _refused(lib.bnerv_fetch_frame(None, _p(0), None, _p(1), 3, 64, _p(2, 4), None), "fetch_frame", "dst_img", "16-byte aligned")
    # an odd frame size puts every frame but the first off the 16-byte grid: refused for a clip, fine for a single frame (checked next)
    _refused(lib.bnerv_fetch_frame(None, _p(0), None, _p(1), 3, 63, _p(2), None), "fetch_frame", "frame_elems")


def test_conv5_refuses_misaligned_shuffled_outputs_and_workspace():
    lib = L.load()

    def desc(out_off=0, out2_off=0, out_s=2):
        return L.ConvDesc(_p(0), _p(1), _p(2), _p(3, out_off), _p(4, out2_off), None, None, None, None, None, None,
                          1, 12, 48, 8, 32, 5, L.IN_PLAIN, L.EP_BIAS_GELU, 1, out_s, 0, 48, 12, None)
    nbytes = lib.bnerv_conv5_ws_bytes(12, 48)
    for d in (desc(out_off=4), desc(out2_off=4), desc(out_off=12)):
        _refused(lib.bnerv_conv5_igemm(None, C.byref(d), _p(5), nbytes), "conv5_igemm", "out", "out2", "8-byte aligned")
    # the workspace holds 16-byte weight fragments; an 8-byte aligned shuffled output passes the output check and reaches this one
    _refused(lib.bnerv_conv5_igemm(None, C.byref(desc(out_off=8)), _p(5, 4), nbytes), "conv5_igemm", "ws", "16-byte aligned")
    _refused(lib.bnerv_conv5_igemm(None, C.byref(desc(out_off=4, out_s=1)), _p(5, 8), nbytes), "conv5_igemm", "ws", "16-byte aligned")


@pytest.mark.parametrize("entry", ["bnerv_loss_fwd_bwd", "bnerv_loss_ssim_fwd_bwd"])
def test_loss_refuses_a_misaligned_workspace(entry):
    lib = L.load()
    ssim = entry.endswith("ssim_fwd_bwd")
    d = L.LossDesc(_p(0, 4), _p(1, 8), _p(2, 12), _p(3), _p(4), _p(5, 4), 1 << 30, 1, 3, 64, 64, 0.7, 0.0, 0.0 if ssim else 0.3, 0.0)
    rc = lib.bnerv_loss_ssim_fwd_bwd(None, C.byref(d), 0.3) if ssim else lib.bnerv_loss_fwd_bwd(None, C.byref(d))
    _refused(rc, "ws", "8-byte aligned")                    # (pred / target / grad at any 4-byte boundary are not an argument error)


def test_partial_rows_depend_on_the_alignment_of_the_conv_operands():
    """bnerv_conv_partial_rows for 30 -> 30 at 9x16 with EP_DGELU_SAVED: aligned operands take the low-resolution family (4x16 tiles: 3
    rows), a shifted x, out or aux sends the layer to the generic kernel (8x32 tiles: 2 rows) -- a caller that sizes the partial buffer
    for one form and launches the other is written past.  The answer must not depend on `partial` itself."""
    lib = L.load()
    H, W = 9, 16
    small = ((H + 3) // 4) * ((W + 15) // 16)
    assert small == 3 and lib.bnerv_conv_tiles(H, W) == 2

    def rows(x=0, out=0, aux0=0, aux1=0, partial=None):
        d = L.ConvDesc(_p(0, x), _p(1), None, _p(2, out), None, _p(3, aux0), _p(4, aux1), None, _p(5), None, partial,
                       1, 30, 30, H, W, 3, L.IN_PLAIN, L.EP_DGELU_SAVED, 1, 1, 1, 30, 30, None)
        return lib.bnerv_conv_partial_rows(C.byref(d))
    assert rows() == small
    for off in (4, 8, 12):
        assert rows(x=off) == rows(out=off) == rows(aux0=off) == rows(aux1=off) == lib.bnerv_conv_tiles(H, W)
    for part in (_p(6), _p(6, 4)):
        assert rows(partial=part) == small and rows(x=4, partial=part) == lib.bnerv_conv_tiles(H, W)


class _DevicePos:
    """Stands in for a [B] fp64 device tensor: ops.time_branch looks at dtype / is_cuda / dim / shape before it looks at the weights."""
    dtype, is_cuda, shape, device = torch.float64, True, (1,), torch.device("cpu")

    def dim(self):
        return 1

    def contiguous(self):
        return self


def test_time_branch_declines_an_unaligned_weight_before_any_device_call(monkeypatch):
    from boosting_nerv_amd import ops
    calls = []
    monkeypatch.setattr(ops._TimeBranch, "apply", staticmethod(lambda *a: calls.append(a) or (None, None)))
    monkeypatch.delenv("BNERV_TIME_BRANCH", raising=False)
    Lv, SH, SO, TH, TO = 80, 256, 64, 64, 32
    z = lambda *sh: torch.zeros(*sh)
    stem = (z(SH, 2 * Lv, 1, 1), z(SH), z(SO, SH, 1, 1), z(SO))
    mk_t = lambda: [z(TH, 2 * Lv, 1, 1), z(TH), z(TO, TH, 1, 1), z(TO)]
    mk_m = lambda: [[z(TO, TO, 1, 1), z(TO), z(12, TO, 1, 1), z(12)] for _ in range(2)]
    bases = torch.ones(Lv)

    def off4(t):                                            # the same shape one element into a flat buffer
        buf = torch.zeros(t.numel() + 8)
        k = 1 + (-(buf.data_ptr() // 4) % 4)                # element index of the first slot at 4 bytes past a 16-byte boundary
        v = buf[k:k + t.numel()].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 and L.f32c(v).data_ptr() == v.data_ptr()
        return v
    assert all(t.data_ptr() % 16 == 0 for t in (*stem, *mk_t(), *[t for m in mk_m() for t in m])), "torch's CPU allocator aligns to 64 bytes"
    assert ops.time_branch(_DevicePos(), bases, stem, tuple(mk_t()), [tuple(m) for m in mk_m()]) is not None and len(calls) == 1
    for where in ("stem_t w0", "stem_t w1", "mlp w1", "mlp w2"):
        st, ms = mk_t(), mk_m()
        if where == "stem_t w0":
            st[0] = off4(st[0])
        elif where == "stem_t w1":
            st[2] = off4(st[2])
        elif where == "mlp w1":
            ms[1][0] = off4(ms[1][0])
        else:
            ms[0][2] = off4(ms[0][2])
        assert ops.time_branch(_DevicePos(), bases, stem, tuple(st), [tuple(m) for m in ms]) is None, where
    assert len(calls) == 1, "a declined call must not reach the library"
