"""Autograd operators of the decoder path.  Every forward/backward here is a sequence of C-ABI calls into
libbnerv_hip.so on torch's current HIP stream; torch supplies device memory, the stream and the autograd graph only.
Every operator accepts any contiguous fp32 tensor, whatever its data_ptr() % 16 (INTEGRATION.md "Pointer alignment").

Operator <-> reference map (the Python modules in this package call these from the same places the reference calls
ATen):
  positional_encoding      PositionEncoding.forward              model_blocks.py:120-126
  dense_grouped            NeRV_MLP / SFTLayer 1x1 convs         model_blocks.py:66-71, :92-105
  conv2d_ps                CustomConv2d (+PixelShuffle)          lib/quant_ops.py:39-41, model_blocks.py:213-218
  upconv_act               NeRVBlock.forward without TAT         model_blocks.py:34-46 (HNeRV baseline: conv + PixelShuffle + GELU)
  snerv_block              NeRVBlock.forward with TAT            model_blocks.py:34-39 + :83-89
  tat_block                ResBlock_SFT.forward                  model_blocks.py:83-89
  sft_affine               SFTLayer.forward (affine part)        model_blocks.py:101-105
  head_tanh                head_layer + OutImg('tanh')           model_nerv.py:56-57, model_blocks.py:57-63
  loss / psnr / msssim     loss_fn, psnr_fn_single, ms_ssim      hnerv_utils.py:335-403, :410-412
  inpaint_head, mask=      TransformInput, loss_fn(out * mask, ..) hnerv_utils.py:59-84, train_nerv_all.py:343
"""
import ctypes as C
import os

import torch
import torch.nn.functional as F

from . import _lib as L


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------------------------------------------------
# raw kernel wrappers
# ----------------------------------------------------------------------------------------------------------------------
_STREAM_CTX = object()      # descriptor builders: "the context of the current stream" (the 5x5 kernels take none: ctx=None)
_SUMS_EP = (L.EP_DGELU, L.EP_DSIN, L.EP_DGELU_SAVED)      # epilogues that also write per-tile (ds, dt) partial sums


def _conv_desc(x, w, bias, out, *, B, Cin, Cout, H, W, k, in_mode, ep_mode, in_s=1, out_s=1, transposed=0, out2=None,
               aux0=None, aux1=None, aux2=None, scale=None, shift=None, partial=None, ctx=_STREAM_CTX):
    """The ConvDesc of include/bnerv.h for one conv launch -- the only place that knows the field order."""
    return L.ConvDesc(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(out), L.ptr(out2), L.ptr(aux0), L.ptr(aux1), L.ptr(aux2),
                      L.ptr(scale), L.ptr(shift), L.ptr(partial), B, Cin, Cout, H, W, k, in_mode, ep_mode, in_s, out_s,
                      transposed, w.shape[0], w.shape[1], L.ctx().handle if ctx is _STREAM_CTX else ctx)


def _wgrad_desc(x, g, dw, db, ws, ws_bytes, *, B, Cin, Cout, H, W, k, in_mode, g_mode, g_s=1, gaux=None, scale=None, shift=None,
                defer=False, ctx=_STREAM_CTX):
    """The WgradDesc of include/bnerv.h for one weight-gradient launch -- the only place that knows the field order."""
    return L.WgradDesc(L.ptr(x), L.ptr(g), L.ptr(gaux), L.ptr(scale), L.ptr(shift), L.ptr(dw), L.ptr(db), L.ptr(ws), ws_bytes,
                       B, Cin, Cout, H, W, k, in_mode, g_mode, g_s, 1 if defer else 0, L.ctx().handle if ctx is _STREAM_CTX else ctx)


def _sums_partial(d, device):
    """The [rows, B, 2, Cout] partial-sum buffer of an EP_DGELU / EP_DSIN / EP_DGELU_SAVED launch, hooked into d.  The kernel (hence
    its tile height) is chosen from shape + alignment -> ask the library for the row count of THIS descriptor."""
    rows = L.load().bnerv_conv_partial_rows(C.byref(d))
    part = torch.empty(rows, d.B, 2, d.Cout, dtype=torch.float32, device=device)
    d.partial = part.data_ptr()
    return part, rows


def _splitk_ws(d, device):
    """The split-K slab workspace of an EP_PLAIN launch (low-resolution, long-K layers), hooked into d; None where the layer wants none."""
    nbytes = L.load().bnerv_conv_splitk_ws_bytes(C.byref(d))
    if not nbytes:
        return None
    ws = _ws(nbytes, device)
    d.partial = ws.data_ptr()
    return ws


def _reduced_sums(part, rows, d, device, defer):
    st = torch.empty(d.B, 2, d.Cout, dtype=torch.float32, device=device)
    _reduce_slabs(part, rows, d.B * 2 * d.Cout, st, defer=defer)
    return st


def _conv(x, w, bias, out, *, B, Cin, Cout, H, W, k, in_mode, ep_mode, in_s=1, out_s=1, transposed=0, out2=None,
          aux0=None, aux1=None, aux2=None, scale=None, shift=None, partial=None, defer=False):
    """One conv launch.  Returns the [B, 2, Cout] channel sums for the _SUMS_EP epilogues, else None."""
    d = _conv_desc(x, w, bias, out, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=in_mode, ep_mode=ep_mode, in_s=in_s, out_s=out_s,
                   transposed=transposed, out2=out2, aux0=aux0, aux1=aux1, aux2=aux2, scale=scale, shift=shift, partial=partial)
    lib = L.load()
    if ep_mode in _SUMS_EP:
        part, rows = _sums_partial(d, x.device)
        L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(d)), "bnerv_conv_igemm")
        return _reduced_sums(part, rows, d, x.device, defer)
    ws = _splitk_ws(d, x.device) if ep_mode == L.EP_PLAIN and partial is None else None      # (held only so the buffer lives until the launch is enqueued)
    L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(d)), "bnerv_conv_igemm")


def _wgrad(x, g, dw, db, *, B, Cin, Cout, H, W, k, in_mode, g_mode, g_s=1, gaux=None, scale=None, shift=None, defer=False):
    lib = L.load()
    nbytes = lib.bnerv_conv_wgrad_ws_bytes(B, Cin, Cout, H, W, k)
    ws = _ws(nbytes, x.device)
    d = _wgrad_desc(x, g, dw, db, ws, nbytes, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=in_mode, g_mode=g_mode, g_s=g_s, gaux=gaux,
                    scale=scale, shift=shift, defer=defer)
    L.check(lib.bnerv_conv_wgrad(L.stream(), C.byref(d)), "bnerv_conv_wgrad")
    if defer:
        L.ctx().keep.append(ws)


def _wgrad_conv_pair(wg, cv):
    """One weight gradient and one data gradient that read the same incoming gradient and do not depend on each other, as ONE launch
    when the library takes the pair (include/bnerv.h bnerv_conv_wgrad_pair: 12-channel 3x3 layers), as the two usual launches
    otherwise.  wg: keyword arguments of _wgrad (x, g, dw, db first), always deferred; cv: keyword arguments of _conv (x, w, bias, out
    first) for an EP_DGELU_SAVED / EP_DSIN / EP_PLAIN epilogue; neither dict is modified.  Returns (what _conv returns: the [B, 2, C]
    channel sums or None, dx_queued: the DATA gradient itself (cv's `out`) is still a queued slab reduction when the call returns --
    the stem pair, csrc/stem.hip; every other form writes `out` directly)."""
    lib = L.load()
    dev = wg["x"].device
    nbytes = lib.bnerv_conv_wgrad_ws_bytes(wg["B"], wg["Cin"], wg["Cout"], wg["H"], wg["W"], wg["k"])
    ws = _ws(nbytes, dev)
    wd = _wgrad_desc(ws=ws, ws_bytes=nbytes, **{**wg, "defer": True})
    cd = _conv_desc(**cv)
    red = cv["ep_mode"] in _SUMS_EP
    skw = None
    if red:
        part, rows = _sums_partial(cd, dev)
    elif cv["ep_mode"] == L.EP_PLAIN:                      # a split-K layer (the stem stage's long-K data gradient): its slab workspace
        skw = _splitk_ws(cd, dev)
    rc = lib.bnerv_conv_wgrad_pair(L.stream(), C.byref(cd), C.byref(wd))
    if rc == 1:                                            # not a pair the launch takes: the two usual calls, weight gradient first
        L.check(lib.bnerv_conv_wgrad(L.stream(), C.byref(wd)), "bnerv_conv_wgrad")
        L.check(lib.bnerv_conv_igemm(L.stream(), C.byref(cd)), "bnerv_conv_igemm")
    else:
        L.check(rc, "bnerv_conv_wgrad_pair")
    dx_queued = rc != 1 and skw is not None                # the stem pair sums its slabs in a deferred reduction: `out` is complete
    if dx_queued:                                          # only after the next flush, and the slabs stay alive until then
        L.ctx().keep.append(skw)
    L.ctx().keep.append(ws)
    return (_reduced_sums(part, rows, cd, dev, True) if red else None), dx_queued


# Deferred slab reductions (include/bnerv.h, bnerv_reduce_slabs_deferred): inside one backward the reductions are queued in the
# CONTEXT of the current stream (L.ctx()) and ride on the next lean conv / weight-gradient launch of that stream; the flush that
# ends the block's backward (_end_block) launches the leftovers, so every tensor a backward returns is complete on the stream.
# The workspaces of queued jobs are kept alive by the context until then.
def _reduce_slabs(slabs, n_slabs, count, out, defer=False):
    if defer:
        c = L.ctx()
        L.check(L.load().bnerv_reduce_slabs_deferred(c.handle, L.stream(), L.ptr(slabs), n_slabs, count, L.ptr(out)), "bnerv_reduce_slabs_deferred")
        c.keep.append(slabs)
        return
    L.check(L.load().bnerv_reduce_slabs(L.stream(), L.ptr(slabs), n_slabs, count, L.ptr(out)), "bnerv_reduce_slabs")


# What is still queued is recorded on the stream context (_lib.StreamContext: keep, dx_queued); here only whether laziness is on
_lazy = []      # one dx_ok per open lazy_flush(), innermost last; empty: every block's backward ends with a flush


def _flush_deferred():
    """Launch whatever slab reductions are still queued on this stream's context (an empty queue launches nothing: bnerv_side_flush)."""
    c = L.ctx()
    L.check(L.load().bnerv_flush_deferred(c.handle, L.stream()), "bnerv_flush_deferred")
    c.keep.clear()
    c.dx_queued = False


def _end_block(dx_queued=False):
    """Close a block's backward with a flush -- skipped inside lazy_flush(), because the queued results (weight / bias gradients, the
    per-channel TAT sums) have no reader until the grouped dense backward or the optimizer, and both flush first: ~5 small dependent
    launches per step less.  `dx_queued`: the block returns a DATA gradient that is itself queued (the stem pair).  Whatever produced
    the block's input reads it: an operator of this package flushes on entry (_enter_backward), a stock torch operator would read the
    unreduced buffer -- so that flush is skipped only under lazy_flush(dx_ok=True), and the context is told.  dx_ok therefore covers
    EVERY block that may take the stem pair: it is right only where the immediate reader of each such gradient is an operator of this
    package (B -> torch.sin -> A would hand sin's backward the unreduced buffer before A's entry flush)."""
    if _lazy and (not dx_queued or _lazy[-1]):
        if dx_queued:
            L.ctx().dx_queued = True
        return
    _flush_deferred()


def _enter_backward(reads_sums=False):
    """First line of every backward of this package: flush if a data gradient was returned queued (_end_block), whoever reads it, and
    -- `reads_sums`: the incoming gradients are themselves deferred results inside lazy_flush(), the TAT blocks' channel sums --
    whenever laziness is on.  Invariant: a flush with an empty queue launches nothing, and in every shipped config the only reader
    of a queued data gradient is a reads_sums operator -- so no shipped config gains or moves a launch through this line."""
    c = L.ctx(create=False)
    if (c is not None and c.dx_queued) or (reads_sums and _lazy):
        _flush_deferred()


class lazy_flush:
    """with lazy_flush(): backward()  -- postpone the end-of-block flushes of the deferred slab reductions; every consumer inside this
    package flushes on entry where it has to (_enter_backward), and leaving the outermost context flushes the rest.
    dx_ok: the model's word that a block whose INPUT gradient may stay queued (_end_block: the stem pair, in shipped configs the first
    block only) is fed directly by an operator of this package."""

    def __init__(self, dx_ok=False):
        self.dx_ok = bool(dx_ok)

    def __enter__(self):
        _lazy.append(self.dx_ok)
        return self

    def __exit__(self, *exc):
        _lazy.pop()
        if not _lazy:
            _flush_deferred()
        return False


def _bc(t, B, Cc):
    """[B,C,1,1] / [B,C] modulation tensor -> contiguous fp32 [B,C]."""
    t = L.f32c(t).reshape(B, Cc)
    return t


# ----------------------------------------------------------------------------------------------------------------------
# positional encoding (no gradient: positions are data)
# ----------------------------------------------------------------------------------------------------------------------
def positional_encoding(pos, bases, round_to_f32=False):
    """pos [N,1] fp32 or fp64 on the device; bases fp32 [L] (built on the host by the reference expression).
    Returns [N, 2L, 1, 1] fp32 = cat[sin(pos*bases), cos(pos*bases)]; fp64 positions use the fp64 product form -- unless
    round_to_f32: then they are rounded to fp32 first, i.e. positional_encoding(pos.float(), bases) without the conversion launch."""
    L.require_device(pos, "pos")
    N, Lv = pos.shape[0], bases.numel()
    bases = bases.to(device=pos.device, dtype=torch.float32).contiguous()
    out = torch.empty(N, 2 * Lv, 1, 1, dtype=torch.float32, device=pos.device)
    lib = L.load()
    if pos.dtype == torch.float64 and round_to_f32:
        L.check(lib.bnerv_pe_fwd_f32_from_f64(L.stream(), L.ptr(pos.contiguous()), L.ptr(bases), L.ptr(out), N, Lv), "bnerv_pe_fwd_f32_from_f64")
    elif pos.dtype == torch.float64:
        L.check(lib.bnerv_pe_fwd_f64(L.stream(), L.ptr(pos.contiguous()), L.ptr(bases), L.ptr(out), N, Lv), "bnerv_pe_fwd_f64")
    else:
        p = pos.contiguous() if pos.dtype == torch.float32 else pos.float().contiguous()
        L.check(lib.bnerv_pe_fwd_f32(L.stream(), L.ptr(p), L.ptr(bases), L.ptr(out), N, Lv), "bnerv_pe_fwd_f32")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# grouped dense layers
# ----------------------------------------------------------------------------------------------------------------------
_ACT = {"none": L.ACT_NONE, None: L.ACT_NONE, "relu": L.ACT_RELU, "sin": L.ACT_SIN}


class _DenseGrouped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, n, *tensors):
        xs, ws, bs = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        lib = L.load()
        B = xs[0].shape[0]
        dev = xs[0].device
        xc, wc, ys, auxs = [], [], [], []
        descs = []
        for i in range(n):
            x = L.f32c(L.require_device(xs[i], "x")).reshape(B, -1)
            w = L.f32c(ws[i]).reshape(ws[i].shape[0], -1)
            b = None if bs[i] is None else L.f32c(bs[i])
            O, I = w.shape
            assert x.shape[1] == I, (x.shape, w.shape)
            y = torch.empty(B, O, dtype=torch.float32, device=dev)
            aux = torch.empty(B, O, dtype=torch.float32, device=dev) if acts[i] == L.ACT_SIN else None
            descs.append(L.DenseFwdDesc(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(aux), I, O, acts[i], 0))
            xc.append(x); wc.append(w); ys.append(y); auxs.append(aux)
        for i0 in range(0, n, L.MAX_DENSE_GROUPS):
            chunk = descs[i0:i0 + L.MAX_DENSE_GROUPS]
            arr = (L.DenseFwdDesc * len(chunk))(*chunk)
            L.check(lib.bnerv_dense_grouped_fwd(L.stream(), arr, len(chunk), B), "bnerv_dense_grouped_fwd")
        ctx.acts, ctx.n, ctx.B = acts, n, B
        ctx.has_b = [b is not None for b in bs]
        ctx.xshapes = [tuple(x.shape) for x in xs]
        ctx.wshapes = [tuple(w.shape) for w in ws]
        ctx.same_x = all(x.data_ptr() == xc[0].data_ptr() and x.shape == xc[0].shape for x in xc)
        ctx.save_for_backward(*xc, *wc, *ys, *auxs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        _enter_backward(reads_sums=True)    # the incoming gradients may be deferred slab reductions (the TAT blocks' channel sums)
        n = ctx.n
        sv = ctx.saved_tensors
        xc, wc, ys, auxs = sv[:n], sv[n:2 * n], sv[2 * n:3 * n], sv[3 * n:4 * n]
        need_x = [ctx.needs_input_grad[2 + i] for i in range(n)]
        dxs, dws, dbs = _dense_grouped_bwd(ctx.acts, xc, wc, ys, auxs, dys, need_x, ctx.has_b, ctx.same_x, ctx.B)
        dws = [dw.reshape(sh) for dw, sh in zip(dws, ctx.wshapes)]
        dxs = [None if dx is None else dx.reshape(sh) for dx, sh in zip(dxs, ctx.xshapes)]
        return (None, None) + tuple(dxs) + tuple(dws) + tuple(dbs)


def _dense_grouped_bwd(acts, xc, wc, ys, auxs, dys, need_x, has_b, same_x, B, defer_reduce=False):
    """Backward of n grouped dense layers y_i = act_i(W_i x_i + b_i) (bnerv_dense_grouped_bwd): returns ([dx_i or None], [dW_i [O, I]], [db_i or
    None]).  same_x: every layer read the SAME input tensor -- its gradient is the sum over the layers, returned in the first needed slot.
    defer_reduce: input gradients that need a slab reduction (shared inputs, layers wider than one dx chunk) are QUEUED on the stream context
    (deferred slab reductions, _reduce_slabs(defer=True)) instead of launched: the caller flushes once for several of them."""
    n = len(xc)
    lib = L.load()
    dev = ys[0].device
    descs, keep = [], []
    dws, dbs, dxps, nchunks = [], [], [], []
    I0 = wc[0].shape[1]
    shared = same_x and n > 1 and any(need_x) and all(w.shape[0] <= L.DENSE_DX_CHUNK and w.shape[1] == I0 for w in wc)
    shared_buf = torch.empty(n, B, I0, dtype=torch.float32, device=dev) if shared else None
    for i in range(n):
        x, w = xc[i], wc[i]
        O, I = w.shape
        dy = dys[i]
        if dy is None:
            dy = torch.zeros(B, O, dtype=torch.float32, device=dev)
        dy = L.f32c(dy).reshape(B, O)
        dw = torch.empty(O, I, dtype=torch.float32, device=dev)
        db = torch.empty(O, dtype=torch.float32, device=dev) if has_b[i] else None
        dpre = torch.empty(B, O, dtype=torch.float32, device=dev)
        nch = (O + L.DENSE_DX_CHUNK - 1) // L.DENSE_DX_CHUNK
        if shared:
            dxp = shared_buf[i]
        elif need_x[i]:
            dxp = torch.empty(nch, B, I, dtype=torch.float32, device=dev)
        else:
            dxp = None
        descs.append(L.DenseBwdDesc(L.ptr(x), L.ptr(w), L.ptr(ys[i]), L.ptr(auxs[i]), L.ptr(dy), L.ptr(dpre), L.ptr(dw), L.ptr(db),
                                    L.ptr(dxp), I, O, acts[i], 0))
        keep.append((dy, dpre))
        dws.append(dw); dbs.append(db); dxps.append(dxp); nchunks.append(nch)
    for i0 in range(0, n, L.MAX_DENSE_GROUPS):
        chunk = descs[i0:i0 + L.MAX_DENSE_GROUPS]
        arr = (L.DenseBwdDesc * len(chunk))(*chunk)
        L.check(lib.bnerv_dense_grouped_bwd(L.stream(), arr, len(chunk), B), "bnerv_dense_grouped_bwd")
    dxs = [None] * n
    if shared:
        tot = torch.empty(B, I0, dtype=torch.float32, device=dev)
        _reduce_slabs(shared_buf, n, B * I0, tot, defer=defer_reduce)
        first = next(i for i in range(n) if need_x[i])
        dxs[first] = tot               # the same tensor was passed n times: its whole gradient goes to one slot
    else:
        for i in range(n):
            if dxps[i] is None:
                continue
            if nchunks[i] == 1:
                dxs[i] = dxps[i][0]
            else:
                I = wc[i].shape[1]
                tot = torch.empty(B, I, dtype=torch.float32, device=dev)
                _reduce_slabs(dxps[i], nchunks[i], B * I, tot, defer=defer_reduce)
                dxs[i] = tot
    return dxs, dws, dbs


DENSE_GEMM_MIN_B = 16


class _DenseGemm(torch.autograd.Function):
    """y = act(x W^T + b) for many rows on the MFMA GEMM kernel (bnerv_dense_gemm_fwd / _bwd, csrc/gemm.hip)."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x2 = L.f32c(L.require_device(x, "x")).reshape(x.shape[0], -1)
        w2 = L.f32c(w).reshape(w.shape[0], -1)
        b2 = None if b is None else L.f32c(b)
        B, I = x2.shape
        O = w2.shape[0]
        assert w2.shape[1] == I, (x.shape, w.shape)
        y = torch.empty(B, O, dtype=torch.float32, device=x2.device)
        aux = torch.empty(B, O, dtype=torch.float32, device=x2.device) if act == L.ACT_SIN else None
        L.check(L.load().bnerv_dense_gemm_fwd(L.stream(), L.ptr(x2), L.ptr(w2), L.ptr(b2), L.ptr(y), L.ptr(aux), B, I, O, act), "bnerv_dense_gemm_fwd")
        ctx.save_for_backward(x2, w2, y, aux)
        ctx.act, ctx.has_b, ctx.xshape, ctx.wshape = act, b is not None, tuple(x.shape), tuple(w.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        _enter_backward(reads_sums=True)
        x2, w2, y, aux = ctx.saved_tensors
        B, I = x2.shape
        O = w2.shape[0]
        dy = L.f32c(dy).reshape(B, O)
        dw = torch.empty(O, I, dtype=torch.float32, device=x2.device)
        db = torch.empty(O, dtype=torch.float32, device=x2.device) if ctx.has_b else None
        dx = torch.empty(B, I, dtype=torch.float32, device=x2.device) if ctx.needs_input_grad[0] else None
        lib = L.load()
        nbytes = lib.bnerv_dense_gemm_bwd_ws_bytes(B, I, O)
        ws = _ws(nbytes, x2.device) if nbytes else None
        L.check(lib.bnerv_dense_gemm_bwd(L.stream(), L.ptr(x2), L.ptr(w2), L.ptr(y), L.ptr(aux), L.ptr(dy), L.ptr(dx), L.ptr(dw), L.ptr(db),
                                         L.ptr(ws), nbytes, B, I, O, ctx.act), "bnerv_dense_gemm_bwd")
        return (None if dx is None else dx.reshape(ctx.xshape)), dw.reshape(ctx.wshape), db, None


def dense_gemm(x, w, b, act="none"):
    """act(x [rows, I] w[O, I]^T + b) -> [rows, O] on the MFMA GEMM kernel (any row count; meant for >= 16 rows)."""
    return _DenseGemm.apply(x, w, b, _ACT[act])


TIME_BRANCH_BWD_CALLS = {"taken": 0, "declined": 0}      # how _TimeBranch.backward's two-launch entry point answered (tests read it)


def _time_branch_bwd_two_launches(B, saved, hs, p2, d_sy1, d_ty1, d_outs):
    """The backward of the whole time branch as two launches (include/bnerv.h bnerv_time_branch_bwd): the gradients of p2 in p2's order
    (flat [O, I] / [O] tensors), or None when the shapes are not the kernels' -- the caller then runs the five grouped launches.  Every
    gradient has the bits of that form.  A d_outs[i] of None (the output took no part in the loss) is zeros, a d_ty1 of None adds nothing."""
    pe, sy0, saux0, sy1, saux1, ty0, taux0, ty1, taux1 = saved
    sw0, sb0, sw1, sb1, tw0, tb0, tw1, tb1 = p2[:8]
    mw = p2[8:]
    n = len(hs)
    dev = pe.device
    SH, SO, TH, TO = sw0.shape[0], sw1.shape[0], tw0.shape[0], tw1.shape[0]
    f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    g = [f(*t.shape) for t in p2]
    nch = (SO + L.DENSE_DX_CHUNK - 1) // L.DENSE_DX_CHUNK
    sx_part, zt_part, s_dpre = f(nch, B, SH), f(n, B, TO), f(B, SO)
    d_sy1 = L.f32c(d_sy1).reshape(B, SO)
    d_ty1 = None if d_ty1 is None else L.f32c(d_ty1).reshape(B, TO)
    douts = [None if t is None else L.f32c(t).reshape(B, -1) for t in d_outs]
    d = L.TimeBranchBwdDesc(L.ptr(pe), L.ptr(sw1), L.ptr(sy0), L.ptr(saux0), L.ptr(saux1), L.ptr(d_sy1),
                            L.ptr(tw1), L.ptr(ty0), L.ptr(taux0), L.ptr(ty1), L.ptr(taux1), L.ptr(d_ty1),
                            L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(g[3]), L.ptr(g[4]), L.ptr(g[5]), L.ptr(g[6]), L.ptr(g[7]),
                            L.ptr(sx_part), L.ptr(zt_part), L.ptr(s_dpre), B, pe.shape[1] // 2, SH, SO, TH, TO, n, 0)
    ml = (L.TimeBranchBwdMlp * n)()
    for i in range(n):
        w1, _, w2, _ = mw[4 * i:4 * i + 4]
        dw1, db1, dw2, db2 = g[8 + 4 * i:12 + 4 * i]
        ml[i].w1, ml[i].w2, ml[i].hs, ml[i].d_out = w1.data_ptr(), w2.data_ptr(), hs[i].data_ptr(), L.ptr(douts[i])
        ml[i].dw1, ml[i].db1, ml[i].dw2, ml[i].db2, ml[i].C = dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), w2.shape[0]
    rc = L.load().bnerv_time_branch_bwd(L.stream(), C.byref(d), ml)
    if rc == 1:
        return None
    L.check(rc, "bnerv_time_branch_bwd")
    return g


class _TimeBranch(torch.autograd.Function):
    """PositionEncoding -> stem layer 0 | stem_t (both layers) -> every TAT modulation MLP as ONE launch (include/bnerv.h
    bnerv_time_branch_fwd), then the stem's second layer as the ordinary grouped launch: 2 launches for the reference's chain of
    model_nerv.py:47-51 / model_blocks.py:92-105 instead of 5.  The backward is two launches as well (bnerv_time_branch_bwd: the stem's
    layer 1 beside both layers of every modulation MLP, then the stem's layer 0 beside stem_t's chain), with the bits of the grouped dense
    backward of the four depths -- which still runs where that entry point declines the shapes, or with BNERV_TIME_BRANCH_BWD=0."""

    @staticmethod
    def forward(ctx, pos, bases, n_mlp, *params):
        lib = L.load()
        dev = pos.device
        B, Lv = pos.shape[0], bases.numel()
        p2 = [L.f32c(t).reshape(t.shape[0], -1) if t.dim() > 1 else L.f32c(t) for t in params]
        sw0, sb0, sw1, sb1, tw0, tb0, tw1, tb1 = p2[:8]
        mw = p2[8:]
        SH, SO, TH, TO = sw0.shape[0], sw1.shape[0], tw0.shape[0], tw1.shape[0]
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        pe, sy0, saux0, sy1, saux1 = f(B, 2 * Lv), f(B, SH), f(B, SH), f(B, SO), f(B, SO)
        ty0, taux0, ty1, taux1 = f(B, TH), f(B, TH), f(B, TO), f(B, TO)
        hs = [f(B, TO) for _ in range(n_mlp)]
        outs = [f(B, mw[4 * i + 2].shape[0]) for i in range(n_mlp)]
        d = L.TimeBranchDesc(L.ptr(pos), L.ptr(bases), L.ptr(pe), L.ptr(sw0), L.ptr(sb0), L.ptr(sy0), L.ptr(saux0),
                             L.ptr(tw0), L.ptr(tb0), L.ptr(tw1), L.ptr(tb1), L.ptr(ty0), L.ptr(taux0), L.ptr(ty1), L.ptr(taux1), B, Lv, SH, TH, TO, n_mlp)
        ml = (L.TimeBranchMlp * max(n_mlp, 1))()
        for i in range(n_mlp):
            w1, b1, w2, b2 = mw[4 * i:4 * i + 4]
            ml[i].w1, ml[i].b1, ml[i].w2, ml[i].b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
            ml[i].hs, ml[i].out, ml[i].C = hs[i].data_ptr(), outs[i].data_ptr(), w2.shape[0]
        rc = lib.bnerv_time_branch_fwd(L.stream(), C.byref(d), ml)
        if rc != 0:
            L.check(rc if rc < 0 else -1, "bnerv_time_branch_fwd (shapes were checked by ops.time_branch)")
        g = (L.DenseFwdDesc * 1)(L.DenseFwdDesc(L.ptr(sy0), L.ptr(sw1), L.ptr(sb1), L.ptr(sy1), L.ptr(saux1), SH, SO, L.ACT_SIN, 0))
        L.check(lib.bnerv_dense_grouped_fwd(L.stream(), g, 1, B), "bnerv_dense_grouped_fwd")
        ctx.n_mlp, ctx.B = n_mlp, B
        ctx.pshapes = [tuple(t.shape) for t in params]
        ctx.save_for_backward(pe, sy0, saux0, sy1, saux1, ty0, taux0, ty1, taux1, *hs, *outs, *p2)
        # z_t has no consumer besides the modulation MLPs when they are all evaluated here: autograd would otherwise materialise a zero
        # gradient for it (a fill launch) and the backward would add it (another launch)
        ctx.set_materialize_grads(False)
        return (sy1, ty1, *outs)

    @staticmethod
    def backward(ctx, d_sy1, d_ty1, *d_outs):
        """After the entry flush, two launches (_time_branch_bwd_two_launches).  Where those decline the shapes, or with
        BNERV_TIME_BRANCH_BWD=0 (read per call), the grouped form they were derived from, whose bits they keep:
        five launches instead of the layer-by-layer backward's six (and one reduction launch instead of two): the branches' levels are
        grouped by what is READY, not by which forward launch they came from --
            [every modulation MLP's layer 1 | the stem's layer 1]  ->  [every MLP's layer 0]  ->  ONE flush of both pending input-gradient
            reductions (z_t's over the 32 MLPs, the stem's 68 chunks)  ->  [stem_t layer 1 | stem layer 0]  ->  [stem_t layer 0]."""
        _enter_backward(reads_sums=True)    # the modulation gradients are deferred slab reductions of the TAT blocks
        n, B = ctx.n_mlp, ctx.B
        sv = ctx.saved_tensors
        pe, sy0, saux0, sy1, saux1, ty0, taux0, ty1, taux1 = sv[:9]
        hs, outs, p2 = sv[9:9 + n], sv[9 + n:9 + 2 * n], sv[9 + 2 * n:]
        sw0, sb0, sw1, sb1, tw0, tb0, tw1, tb1 = p2[:8]
        mw = p2[8:]
        none, relu, sin = L.ACT_NONE, L.ACT_RELU, L.ACT_SIN
        g = [None] * len(p2)
        w1s, w2s = [mw[4 * i] for i in range(n)], [mw[4 * i + 2] for i in range(n)]
        if n + 1 > L.MAX_DENSE_GROUPS or n == 0:
            raise L.BnervError("time branch backward: group count outside the grouped kernel's table")
        if os.environ.get("BNERV_TIME_BRANCH_BWD", "1") != "0":
            g2 = _time_branch_bwd_two_launches(B, sv[:9], hs, p2, d_sy1, d_ty1, d_outs)
            TIME_BRANCH_BWD_CALLS["taken" if g2 is not None else "declined"] += 1
            if g2 is not None:
                return (None, None, None, *[t.reshape(sh) for t, sh in zip(g2, ctx.pshapes)])
        # level 1: layer 1 of every modulation MLP + the stem's layer 1 (its input gradient: 68 chunks, reduced below)
        dxa, dwa, dba = _dense_grouped_bwd([none] * n + [sin], list(hs) + [sy0], w2s + [sw1], list(outs) + [sy1], [None] * n + [saux1],
                                           list(d_outs) + [d_sy1], [True] * (n + 1), [True] * (n + 1), False, B, defer_reduce=True)
        dx4, d_sy0 = dxa[:n], dxa[n]
        if any(w.shape[0] > L.DENSE_DX_CHUNK for w in w2s):
            # a modulation MLP wider than one dx chunk (C_i in 65..128): its hidden-layer gradient dx4[i] is itself a queued slab
            # reduction, and level 2 reads it -- reduce now (one more launch, only for such widths; C1 / C4 widths are <= 59)
            _flush_deferred()
        # level 2: layer 0 of every MLP (all read z_t: one shared gradient, summed over the MLPs below)
        dx3, dw3, db3 = _dense_grouped_bwd([relu] * n, [ty1] * n, w1s, hs, [None] * n, dx4, [True] * n, [True] * n, True, B, defer_reduce=True)
        _flush_deferred()                   # both reductions (and whatever else was still queued) in ONE launch
        tot = next(t for t in dx3 if t is not None)
        d_zt = tot if d_ty1 is None else tot + L.f32c(d_ty1).reshape(tot.shape)
        for i in range(n):
            g[8 + 4 * i], g[8 + 4 * i + 1], g[8 + 4 * i + 2], g[8 + 4 * i + 3] = dw3[i], db3[i], dwa[i], dba[i]
        # level 3: stem_t's layer 1 and the stem's layer 0 (the positional encoding has no gradient)
        dxb, dwb, dbb = _dense_grouped_bwd([sin, sin], [ty0, pe], [tw1, sw0], [ty1, sy0], [taux1, saux0], [d_zt, d_sy0], [True, False], [True, True], False, B)
        # level 4: stem_t's layer 0
        _, dwc, dbc = _dense_grouped_bwd([sin], [pe], [tw0], [ty0], [taux0], [dxb[0]], [False], [True], False, B)
        g[0], g[1], g[2], g[3] = dwb[1], dbb[1], dwa[n], dba[n]
        g[4], g[5], g[6], g[7] = dwc[0], dbc[0], dwb[0], dbb[0]
        g = [None if t is None else t.reshape(sh) for t, sh in zip(g, ctx.pshapes)]
        return (None, None, None, *g)


def time_branch(pos, bases, stem, stem_t, mlps):
    """pos [B] fp64, bases fp32 [L]; stem / stem_t = (w0, b0, w1, b1) of the two 2-layer sin MLPs; mlps = [(w1, b1, w2, b2), ...] of the TAT
    modulation branches (relu inside).  Returns (stem_out [B, SO], z_t [B, TO], [out_i [B, C_i]]), or None when the shapes are not the
    kernel's (the caller runs the five grouped launches).  BNERV_TIME_BRANCH=0 switches it off (A/B).  The backward of the returned
    tensors is two launches (bnerv_time_branch_bwd); BNERV_TIME_BRANCH_BWD=0 runs it as the five grouped launches, same bits (A/B)."""
    if os.environ.get("BNERV_TIME_BRANCH", "1") == "0" or pos.dtype != torch.float64 or not pos.is_cuda or pos.dim() != 1:
        return None
    B, Lv = pos.shape[0], bases.numel()
    if any(t is None for t in (*stem, *stem_t)) or any(t is None for m in mlps for t in m):
        return None
    fl = lambda t: t.reshape(t.shape[0], -1).shape
    SH, TH, TO = stem[0].shape[0], stem_t[0].shape[0], stem_t[2].shape[0]
    # (the backward groups every MLP's layer 1 WITH the stem's layer 1 in one grouped launch: n + 1 groups)
    if B > 4 or 2 * Lv > 256 or (2 * Lv) % 4 or TH > 64 or TH % 4 or TO > 32 or TO % 4 or len(mlps) + 1 > L.MAX_DENSE_GROUPS:
        return None
    # every layer must have the width the kernel indexes with (an SFTLayer built with factor != 1 has a narrower hidden layer)
    if fl(stem[0])[1] != 2 * Lv or fl(stem_t[0])[1] != 2 * Lv or fl(stem[2])[1] != SH or fl(stem_t[2])[1] != TH:
        return None
    if any(fl(m[0]) != (TO, TO) or fl(m[2])[1] != TO or fl(m[2])[0] > 128 for m in mlps):
        return None
    if any(t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 for t in (stem_t[0], stem_t[2], *[m[0] for m in mlps], *[m[2] for m in mlps])):
        return None
    flat = [t for m in mlps for t in m]
    out = _TimeBranch.apply(pos.contiguous(), bases.to(device=pos.device, dtype=torch.float32).contiguous(), len(mlps), *stem, *stem_t, *flat)
    return out[0], out[1], list(out[2:])


def dense_grouped(xs, ws, bs, acts):
    """Evaluate n independent dense layers y_i = act_i(W_i x_i + b_i).
    xs[i]: [B, I_i(,1,1)], ws[i]: [O_i, I_i(,1,1)], bs[i]: [O_i] or None, acts[i] in {'none','relu','sin'}.
    Returns a list of [B, O_i] tensors.  B = 1 per GPU (the reference's batch) is a set of GEMVs and goes to the grouped kernel in
    ONE launch; layers applied to 16 or more rows (E-NeRV's 144-token MLPs) are GEMMs and go to the MFMA GEMM kernel."""
    n = len(xs)
    if xs[0].shape[0] >= DENSE_GEMM_MIN_B:
        return [dense_gemm(x, w, b, act if act is not None else "none") for x, w, b, act in zip(xs, ws, bs, acts)]
    a = tuple(_ACT[x] for x in acts)
    return list(_DenseGrouped.apply(a, n, *xs, *ws, *bs))


# ----------------------------------------------------------------------------------------------------------------------
# plain conv (+ bias, + optional pixel shuffle)
# ----------------------------------------------------------------------------------------------------------------------
class _Conv2dPS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, s):
        x = L.f32c(L.require_device(x, "x")); w = L.f32c(w); b = None if b is None else L.f32c(b)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[-1]
        out = torch.empty(B, Cout // (s * s), H * s, W * s, dtype=torch.float32, device=x.device)
        _conv(x, w, b, out, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS, out_s=s)
        ctx.save_for_backward(x, w)
        ctx.s, ctx.has_b = s, b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        _enter_backward()
        x, w = ctx.saved_tensors
        dx, dw, db = _conv_ps_backward(x, w, L.f32c(g), ctx.s, ctx.has_b, ctx.needs_input_grad[0])
        return dx, dw, db, None


def _conv_ps_backward(x, w, g, s, has_b, need_dx):
    """Backward of conv (k in {1,3}) + bias + PixelShuffle(s) from the gradient g of the shuffled output: (dx or None, dw, db or None).
    The one place that chooses between the (dW | dx) pair and the two launches; it ENDS the block's backward (_end_block)."""
    B, Cin, H, W = x.shape
    Cout, k = w.shape[0], w.shape[-1]
    dw = torch.empty_like(w)
    db = torch.empty(Cout, dtype=torch.float32, device=x.device) if has_b else None
    dx = None
    dxq = False
    if need_dx and k == 3:                                     # (dW | dx): one launch where the library pairs them
        dx = torch.empty_like(x)
        _, dxq = _wgrad_conv_pair(dict(x=x, g=g, dw=dw, db=db, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE, g_s=s),
                                  dict(x=g, w=w, bias=None, out=dx, B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=k, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=s, transposed=1))
    else:
        _wgrad(x, g, dw, db, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE, g_s=s, defer=True)
        if need_dx:
            dx = torch.empty_like(x)
            _conv(g, w, None, dx, B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=k, in_mode=L.IN_UNSHUFFLE, ep_mode=L.EP_PLAIN, in_s=s, transposed=1)
    _end_block(dxq)
    return dx, dw, db


def conv2d_ps(x, w, b, shuffle=1):
    """F.conv2d(x, w, b, stride 1, padding (k-1)//2) followed by PixelShuffle(shuffle); k in {1,3}, and k = 5 through upconv_act."""
    if w.shape[-1] == 5:
        return upconv_act(x, w, b, shuffle, "none")
    return _Conv2dPS.apply(x, w, b, int(shuffle))


# ----------------------------------------------------------------------------------------------------------------------
# up-conv block of the HNeRV baseline: conv (k in {1,3,5}) + bias + PixelShuffle + activation (none | gelu)
# ----------------------------------------------------------------------------------------------------------------------
def _conv5(x, w, bias, out, *, B, Cin, Cout, H, W, in_mode=L.IN_PLAIN, ep_mode, in_s=1, out_s=1, transposed=0, out2=None, aux0=None):
    lib = L.load()
    nbytes = lib.bnerv_conv5_ws_bytes(Cin, Cout)
    ws = _ws(nbytes, x.device)
    d = _conv_desc(x, w, bias, out, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=5, in_mode=in_mode, ep_mode=ep_mode, in_s=in_s, out_s=out_s,
                   transposed=transposed, out2=out2, aux0=aux0, ctx=None)
    L.check(lib.bnerv_conv5_igemm(L.stream(), C.byref(d), L.ptr(ws), nbytes), "bnerv_conv5_igemm")


def _wgrad5(x, g, dw, db, *, B, Cin, Cout, H, W, g_s=1, gaux=None):
    lib = L.load()
    nbytes = lib.bnerv_conv5_wgrad_ws_bytes(B, Cin, Cout, H, W)
    ws = _ws(nbytes, x.device)
    d = _wgrad_desc(x, g, dw, db, ws, nbytes, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=5, in_mode=L.IN_PLAIN,
                    g_mode=L.IN_UNSHUFFLE if g_s > 1 else L.IN_PLAIN, g_s=g_s, gaux=gaux, ctx=None)
    L.check(lib.bnerv_conv5_wgrad(L.stream(), C.byref(d)), "bnerv_conv5_wgrad")


UPCONV_ACTS = ("none", "gelu")


class _UpConvAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, s, act):
        x = L.f32c(L.require_device(x, "x")); w = L.f32c(w); b = None if b is None else L.f32c(b)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[-1]
        gelu = act == "gelu"
        train = any(ctx.needs_input_grad)                   # False under torch.no_grad(): decode keeps no gelu'
        out = torch.empty(B, Cout // (s * s), H * s, W * s, dtype=torch.float32, device=x.device)
        gp = torch.empty_like(out) if (gelu and train) else None
        if k == 5:
            _conv5(x, w, b, out, B=B, Cin=Cin, Cout=Cout, H=H, W=W, ep_mode=L.EP_BIAS_GELU if gelu else L.EP_BIAS, out_s=s, out2=gp)
        else:
            _conv(x, w, b, out, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS, out_s=s)
            if gelu:
                L.check(L.load().bnerv_gelu_fwd(L.stream(), L.ptr(out), L.ptr(out), L.ptr(gp), out.numel()), "bnerv_gelu_fwd")
        if train:
            ctx.save_for_backward(x, w, gp)
        ctx.s, ctx.has_b = s, b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        _enter_backward()
        x, w, gp = ctx.saved_tensors
        s = ctx.s
        g = L.f32c(g)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[-1]
        if k != 5:
            if gp is not None:
                du = torch.empty_like(g)
                L.check(L.load().bnerv_mul(L.stream(), L.ptr(g), L.ptr(gp), L.ptr(du), g.numel()), "bnerv_mul")
                g = du
            dx, dw, db = _conv_ps_backward(x, w, g, s, ctx.has_b, ctx.needs_input_grad[0])
            return dx, dw, db, None, None
        # 5x5: the product with the saved gelu' is folded into the gradient staging of both kernels (du is never written out)
        dw = torch.empty_like(w)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if ctx.has_b else None
        _wgrad5(x, g, dw, db, B=B, Cin=Cin, Cout=Cout, H=H, W=W, g_s=s, gaux=gp)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _conv5(g, w, None, dx, B=B, Cin=Cout, Cout=Cin, H=H, W=W, in_mode=L.IN_UNSHUFFLE if s > 1 else L.IN_PLAIN, ep_mode=L.EP_PLAIN,
                   in_s=s, transposed=1, aux0=gp)
        return dx, dw, db, None, None


def upconv_act(x, w, b, stride=1, act="none"):
    """act(PixelShuffle_stride(F.conv2d(x, w, b, padding (k-1)//2))) -- NeRVBlock.forward of the HNeRV baseline (norm='none'); k in {1,3,5},
    act in {"none", "gelu"}.  5x5: stride in {1, 2}, GELU fused into the conv's epilogue and its derivative into the backward's staging."""
    k = w.shape[-1]
    if act not in UPCONV_ACTS:
        raise NotImplementedError(f"upconv_act: act={act!r} (supported: {UPCONV_ACTS})")
    if w.shape[-2] != k or k not in (1, 3, 5) or (k == 5 and int(stride) not in (1, 2)) or w.shape[0] % (int(stride) ** 2):
        raise NotImplementedError(f"upconv_act: weight {tuple(w.shape)} with stride {stride} is not on the HIP path (k in {{1,3,5}}; 5x5: stride 1 or 2)")
    return _UpConvAct.apply(x, w, b, int(stride), act)


# ----------------------------------------------------------------------------------------------------------------------
# TAT residual block and the fused SNeRV block
# ----------------------------------------------------------------------------------------------------------------------
def _tat_forward(y0, s0, t0, s1, t1, w0, b0, w1, b1, train=True):
    B, Cc, H, W = y0.shape
    # conv0's epilogue stores h = gelu(v) and gp = gelu'(v) instead of v: conv1, its weight gradient and the dGELU epilogue of
    # the backward then run without erf/exp (v itself has no other consumer)
    out = torch.empty_like(y0)
    hs = torch.empty_like(y0) if train else None
    gp = torch.empty_like(y0) if train else None          # decode / eval (no_grad): neither h nor gelu' is read again, so they are not written
    h = hs if train else torch.empty_like(y0)
    _conv(y0, w0, b0, h, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_GELU, scale=s0, shift=t0, out2=gp)
    _conv(h, w1, b1, out, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_AFFINE, ep_mode=L.EP_BIAS_RES, scale=s1, shift=t1, aux0=y0)
    return h, gp, out


def _tat_backward(dout, y0, c0, h, gp, s0, t0, s1, t1, w0, w1):
    """Returns (dy0_or_du, ds0, dt0, ds1, dt1, dw0, db0, dw1, db1).  With c0 given the first result is
    d/d(pre-sin) = (dout + dA0*(1+s0)) * c0, otherwise d/dy0."""
    B, Cc, H, W = y0.shape
    dev = y0.device
    dw1 = torch.empty_like(w1); db1 = torch.empty(Cc, dtype=torch.float32, device=dev)
    # every slab reduction below is deferred: it rides on the next launch of this chain; the CALLER flushes the leftovers
    # (dW1 | d conv1) and (dW0 | d conv0): each pair reads one incoming gradient and is ONE launch where the library pairs them
    dv = torch.empty_like(y0)
    st1, _ = _wgrad_conv_pair(dict(x=h, g=dout, dw=dw1, db=db1, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_AFFINE, g_mode=L.IN_UNSHUFFLE, scale=s1, shift=t1),
                              dict(x=dout, w=w1, bias=None, out=dv, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_PLAIN, ep_mode=L.EP_DGELU_SAVED,
                                   transposed=1, aux0=gp, aux1=h, scale=s1))
    dw0 = torch.empty_like(w0); db0 = torch.empty(Cc, dtype=torch.float32, device=dev)
    du = torch.empty_like(y0)
    st0, _ = _wgrad_conv_pair(dict(x=y0, g=dv, dw=dw0, db=db0, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_AFFINE, g_mode=L.IN_UNSHUFFLE, scale=s0, shift=t0),
                              dict(x=dv, w=w0, bias=None, out=du, B=B, Cin=Cc, Cout=Cc, H=H, W=W, k=3, in_mode=L.IN_PLAIN, ep_mode=L.EP_DSIN,
                                   transposed=1, aux0=y0, aux1=dout, aux2=c0, scale=s0))
    return du, st0[:, 0], st0[:, 1], st1[:, 0], st1[:, 1], dw0, db0, dw1, db1


class _TATBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, s0, t0, s1, t1, w0, b0, w1, b1):
        x0 = L.f32c(L.require_device(x0, "x0"))
        B, Cc = x0.shape[:2]
        s0, t0, s1, t1 = (_bc(t, B, Cc) for t in (s0, t0, s1, t1))
        w0, b0, w1, b1 = (L.f32c(t) for t in (w0, b0, w1, b1))
        train = any(ctx.needs_input_grad)                   # False under torch.no_grad(): the decode path keeps nothing for backward
        h, gp, out = _tat_forward(x0, s0, t0, s1, t1, w0, b0, w1, b1, train)
        if train:
            ctx.save_for_backward(x0, h, gp, s0, t0, s1, t1, w0, w1)
        ctx.mshape = (B, Cc, 1, 1)
        return out

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        x0, h, gp, s0, t0, s1, t1, w0, w1 = ctx.saved_tensors
        dx0, ds0, dt0, ds1, dt1, dw0, db0, dw1, db1 = _tat_backward(L.f32c(dout), x0, None, h, gp, s0, t0, s1, t1, w0, w1)
        _end_block()
        m = ctx.mshape
        return dx0, ds0.reshape(m), dt0.reshape(m), ds1.reshape(m), dt1.reshape(m), dw0, db0, dw1, db1


def tat_block(x0, scale0, shift0, scale1, shift1, w0, b0, w1, b1):
    """x0 + conv1(sft1(gelu(conv0(sft0(x0)))))  with sft_i(a) = a*(scale_i+1)+shift_i  (ResBlock_SFT.forward)."""
    return _TATBlock.apply(x0, scale0, shift0, scale1, shift1, w0, b0, w1, b1)


class _SNeRVBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wu, bu, s0, t0, s1, t1, w0, b0, w1, b1, stride):
        x = L.f32c(L.require_device(x, "x"))
        wu, w0, b0, w1, b1 = (L.f32c(t) for t in (wu, w0, b0, w1, b1))
        bu = None if bu is None else L.f32c(bu)
        B, Cin, H, W = x.shape
        Ct, k = wu.shape[0], wu.shape[-1]
        s = stride
        Cc = Ct // (s * s)
        s0, t0, s1, t1 = (_bc(t, B, Cc) for t in (s0, t0, s1, t1))
        train = any(ctx.needs_input_grad)                   # False under torch.no_grad(): decode path, nothing saved
        y0 = torch.empty(B, Cc, H * s, W * s, dtype=torch.float32, device=x.device)
        c0 = torch.empty_like(y0) if train else None
        _conv(x, wu, bu, y0, B=B, Cin=Cin, Cout=Ct, H=H, W=W, k=k, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS_SIN, out_s=s, out2=c0)
        h, gp, out = _tat_forward(y0, s0, t0, s1, t1, w0, b0, w1, b1, train)
        if train:
            ctx.save_for_backward(x, y0, c0, h, gp, s0, t0, s1, t1, wu, w0, w1)
        ctx.s, ctx.has_bu, ctx.mshape = s, bu is not None, (B, Cc, 1, 1)
        return out

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        x, y0, c0, h, gp, s0, t0, s1, t1, wu, w0, w1 = ctx.saved_tensors
        du, ds0, dt0, ds1, dt1, dw0, db0, dw1, db1 = _tat_backward(L.f32c(dout), y0, c0, h, gp, s0, t0, s1, t1, w0, w1)
        dx, dwu, dbu = _conv_ps_backward(x, wu, du, ctx.s, ctx.has_bu, ctx.needs_input_grad[0])
        m = ctx.mshape
        return dx, dwu, dbu, ds0.reshape(m), dt0.reshape(m), ds1.reshape(m), dt1.reshape(m), dw0, db0, dw1, db1, None


def snerv_block(x, w_up, b_up, scale0, shift0, scale1, shift1, w0, b0, w1, b1, stride):
    """tat_block(sin(PixelShuffle_stride(conv(x, w_up, b_up))))  -- NeRVBlock.forward with act='sin', norm='none'."""
    return _SNeRVBlock.apply(x, w_up, b_up, scale0, shift0, scale1, shift1, w0, b0, w1, b1, int(stride))


# ----------------------------------------------------------------------------------------------------------------------
# stand-alone TAT affine
# ----------------------------------------------------------------------------------------------------------------------
class _SFTAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift):
        x = L.f32c(L.require_device(x, "x"))
        B, Cc = x.shape[:2]
        HW = x[0, 0].numel()
        sc, sh = _bc(scale, B, Cc), _bc(shift, B, Cc)
        y = torch.empty_like(x)
        L.check(L.load().bnerv_sft_affine_fwd(L.stream(), L.ptr(x), L.ptr(sc), L.ptr(sh), L.ptr(y), B, Cc, HW), "bnerv_sft_affine_fwd")
        ctx.save_for_backward(x, sc)
        ctx.mshape = tuple(scale.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        _enter_backward(reads_sums=True)
        x, sc = ctx.saved_tensors
        g = L.f32c(g)
        B, Cc = x.shape[:2]
        HW = x[0, 0].numel()
        dx = torch.empty_like(x)
        part = torch.empty(L.SFT_CHUNKS, 2, B * Cc, dtype=torch.float32, device=x.device)
        L.check(L.load().bnerv_sft_affine_bwd(L.stream(), L.ptr(x), L.ptr(sc), L.ptr(g), L.ptr(dx), L.ptr(part), B, Cc, HW), "bnerv_sft_affine_bwd")
        tot = torch.empty(2, B * Cc, dtype=torch.float32, device=x.device)
        _reduce_slabs(part, L.SFT_CHUNKS, 2 * B * Cc, tot)
        return dx, tot[0].reshape(ctx.mshape), tot[1].reshape(ctx.mshape)


def sft_affine(x, scale, shift):
    return _SFTAffine.apply(x, scale, shift)


# ----------------------------------------------------------------------------------------------------------------------
# head conv + OutImg('tanh')
# ----------------------------------------------------------------------------------------------------------------------
class _HeadTanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = L.f32c(L.require_device(x, "x")); w = L.f32c(w); b = None if b is None else L.f32c(b)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[-1]
        img = torch.empty(B, Cout, H, W, dtype=torch.float32, device=x.device)
        _conv(x, w, b, img, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, ep_mode=L.EP_BIAS_TANH)
        ctx.save_for_backward(x, w, img)
        ctx.has_b = b is not None
        return img

    @staticmethod
    def backward(ctx, g):
        _enter_backward()
        x, w, img = ctx.saved_tensors
        g = L.f32c(g)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[-1]
        dw = torch.empty_like(w)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if ctx.has_b else None
        dx = None
        if k == 3 and Cout <= 4 and Cin >= 16 and os.environ.get("BNERV_HEAD_SWAP", "1") != "0":
            # HNeRV_Boost's 3x3 head (38 -> 3, model_hnerv.py:214).  As dW[co] = sum_p gt[co][p] x[.][p + tap] the MFMA tile has 3 of its 16
            # rows in use (272 us at 1080p).  The same sums with the ROLES SWAPPED -- x as the "gradient" (M = 38 input channels), gt as the
            # "input" (N = 3 couts x 9 taps) -- are S[ci][co][t'] = sum_q x[ci][q] gt[co][q + t' - 1] = dW[co][ci][2 - t'] (zero padding
            # excludes the same terms on both sides): one weight-gradient launch on the well-filled shape, then a transpose + tap flip of
            # 1026 numbers.  gt = the tanh-gradient as a tensor (bnerv_tanh_grad), whose channel sums are the bias gradient.
            lib = L.load()
            HW = H * W
            gt = torch.empty_like(g)
            nblk = lib.bnerv_tanh_grad_blocks(HW)
            part = torch.empty(B * nblk, Cout, dtype=torch.float32, device=x.device)
            L.check(lib.bnerv_tanh_grad(L.stream(), L.ptr(g), L.ptr(img), L.ptr(gt), L.ptr(part), B, Cout, HW), "bnerv_tanh_grad")
            if db is not None:
                _reduce_slabs(part, B * nblk, Cout, db, defer=True)
            sw = torch.empty(Cin, Cout, k, k, dtype=torch.float32, device=x.device)
            sb = torch.empty(Cin, dtype=torch.float32, device=x.device)           # (the swapped call's "bias gradient": channel sums of x, unused)
            _wgrad(gt, x, sw, sb, B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=k, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE)
            dw = sw.permute(1, 0, 2, 3).flip(2, 3).contiguous()
            if ctx.needs_input_grad[0]:           # (gt is a tensor now: the data gradient reads 3 planes instead of 6 -- csrc/head3.hip, 78 against 91 us at 1080p)
                dx = torch.empty_like(x)
                _conv(gt, w, None, dx, B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=k, in_mode=L.IN_PLAIN, ep_mode=L.EP_PLAIN, transposed=1)
        elif ctx.needs_input_grad[0]:
            # (dW | dx) of the head: one streaming pass where the library pairs them (1x1, tanh-grad prologue), the two launches otherwise
            # (never the stem pair, which takes no tanh-grad prologue: this dx is written directly)
            dx = torch.empty_like(x)
            _wgrad_conv_pair(dict(x=x, g=g, dw=dw, db=db, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, g_mode=L.IN_TANHGRAD, gaux=img),
                             dict(x=g, w=w, bias=None, out=dx, B=B, Cin=Cout, Cout=Cin, H=H, W=W, k=k, in_mode=L.IN_TANHGRAD, ep_mode=L.EP_PLAIN, transposed=1, aux0=img))
        else:
            _wgrad(x, g, dw, db, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, in_mode=L.IN_PLAIN, g_mode=L.IN_TANHGRAD, gaux=img, defer=True)
        _end_block()
        return dx, dw, db


def head_tanh(x, w, b):
    """tanh(conv(x, w, b)) * 0.5 + 0.5   (head_layer followed by OutImg(..., 'tanh'))."""
    return _HeadTanh.apply(x, w, b)


# ----------------------------------------------------------------------------------------------------------------------
# CEM compression path: fused quantise + rate term over all weight / bias tensors (row N2)
# ----------------------------------------------------------------------------------------------------------------------
class _CemScaleRate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, training, *tensors):
        ws, scales, noises = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        lib = L.load()
        dev = ws[0].device
        wc = [L.f32c(L.require_device(w, "w")) for w in ws]
        sc = [L.f32c(s) for s in scales]
        nz = [None if z is None else L.f32c(z) for z in noises]
        deq = [torch.empty_like(w) for w in wc]
        stats = torch.empty(n, 4, dtype=torch.float32, device=dev)
        for i0 in range(0, n, L.CEM_MAX_TENSORS):
            ck = L.CemChunk()
            m = min(L.CEM_MAX_TENSORS, n - i0)
            for j in range(m):
                i = i0 + j
                assert sc[i].numel() == 1, "the fused CEM kernel handles per-tensor scales"
                ck.it[j].w, ck.it[j].scale, ck.it[j].dequant, ck.it[j].n = wc[i].data_ptr(), sc[i].data_ptr(), deq[i].data_ptr(), wc[i].numel()
                ck.it[j].noise = nz[i].data_ptr() if nz[i] is not None else None
            ck.n_items, ck.training, ck.first = m, int(training), i0
            nb = lib.bnerv_cem_ws_bytes(m, max(wc[i0 + j].numel() for j in range(m)))
            ws_ = _ws(nb, dev)                                 # chunk partial sums (stream-ordered allocation: reused by the next group)
            L.check(lib.bnerv_cem_scale_fwd(L.stream(), C.byref(ck), L.ptr(stats), L.ptr(ws_), nb), "bnerv_cem_scale_fwd")
        ctx.n, ctx.training = n, training
        ctx.save_for_backward(stats, *wc, *sc, *[z for z in nz if z is not None])
        ctx.has_noise = [z is not None for z in nz]
        ctx.wshapes = [tuple(w.shape) for w in ws]
        ctx.mark_non_differentiable(stats)
        bits = stats[:, 0].clone()
        return (bits, stats, *deq)

    @staticmethod
    def backward(ctx, d_bits, _d_stats, *d_deq):
        _enter_backward()
        n = ctx.n
        sv = ctx.saved_tensors
        stats, wc, sc = sv[0], sv[1:1 + n], sv[1 + n:1 + 2 * n]
        rest = list(sv[1 + 2 * n:])
        nz = [rest.pop(0) if h else None for h in ctx.has_noise]
        lib = L.load()
        dev = stats.device
        d_bits = None if d_bits is None else L.f32c(d_bits)
        dds = [None if g is None else L.f32c(g) for g in d_deq]
        dws = [torch.empty_like(w) for w in wc]
        dscale = torch.empty(n, dtype=torch.float32, device=dev)
        for i0 in range(0, n, L.CEM_MAX_TENSORS):
            ck = L.CemChunkBwd()
            m = min(L.CEM_MAX_TENSORS, n - i0)
            for j in range(m):
                i = i0 + j
                ck.it[j].w, ck.it[j].scale, ck.it[j].dw, ck.it[j].n = wc[i].data_ptr(), sc[i].data_ptr(), dws[i].data_ptr(), wc[i].numel()
                ck.it[j].noise = nz[i].data_ptr() if nz[i] is not None else None
                ck.it[j].d_dequant = dds[i].data_ptr() if dds[i] is not None else None
            ck.n_items, ck.training, ck.first = m, int(ctx.training), i0
            nb = lib.bnerv_cem_ws_bytes(m, max(wc[i0 + j].numel() for j in range(m)))
            ws_ = _ws(nb, dev)
            L.check(lib.bnerv_cem_scale_bwd(L.stream(), C.byref(ck), L.ptr(stats), L.ptr(d_bits), L.ptr(dscale), L.ptr(ws_), nb), "bnerv_cem_scale_bwd")
        gs = [dscale[i:i + 1].reshape(sc[i].shape) for i in range(n)]
        return (None, None, *[dw.reshape(sh) for dw, sh in zip(dws, ctx.wshapes)], *gs, *([None] * n))


def cem_scale_rate(ws, scales, noises, training):
    """Scale_T quantise + Gaussian rate for a list of tensors in one fused pass (include/bnerv.h, bnerv_cem_scale_fwd).
    Returns (bits [n], stats [n,4] = {bits, mean, std, numel}, [dequant_i]).  noises: list of U(-.5,.5) tensors (training) or Nones."""
    n = len(ws)
    out = _CemScaleRate.apply(n, bool(training), *ws, *scales, *noises)
    return out[0], out[1], list(out[2:])


# ----------------------------------------------------------------------------------------------------------------------
# bitstream decoder (codec.py): symbols -> parameters, decoded frame -> interleaved bytes (csrc/codec.hip)
# ----------------------------------------------------------------------------------------------------------------------
def dequant_table(symbols, outs, scales, betas=None):
    """outs[i][...] = symbols[i].float() * scales[i]  (+ betas[i] where given), written IN PLACE with the bits of torch's `quant * scale`
    (`+ beta`): Scale_T / ScaleBeta_T de-quantisation of int32 symbol tensors, <= CEM_MAX_TENSORS tensors per launch.  symbols / outs:
    contiguous int32 / fp32 device tensors of equal numel (views at any 4-byte offset are fine); scales / betas: 1-element fp32 device
    tensors (betas: None, or a list with None entries)."""
    n = len(symbols)
    betas = [None] * n if betas is None else betas
    if not (len(outs) == len(scales) == len(betas) == n):
        raise ValueError("dequant_table: symbols, outs, scales and betas must have one entry per tensor")
    for i in range(n):
        q, o = L.require_device(symbols[i], "symbols"), L.require_device(outs[i], "out")
        if q.dtype != torch.int32 or o.dtype != torch.float32 or not q.is_contiguous() or not o.is_contiguous() or q.numel() != o.numel() or q.numel() == 0:
            raise ValueError(f"dequant_table: item {i}: need non-empty contiguous int32 symbols and an fp32 output of the same numel "
                             f"(got {q.dtype} {tuple(q.shape)}, {o.dtype} {tuple(o.shape)})")
        for t, what in ((scales[i], "scale"), (betas[i], "beta")):
            if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or not t.is_cuda):
                raise ValueError(f"dequant_table: item {i}: {what} must be a 1-element fp32 device tensor (per-tensor quantisers only)")
    lib = L.load()
    for i0 in range(0, n, L.CEM_MAX_TENSORS):
        ck = L.DequantChunk()
        m = min(L.CEM_MAX_TENSORS, n - i0)
        for j in range(m):
            i = i0 + j
            ck.it[j].q, ck.it[j].out, ck.it[j].scale, ck.it[j].n = symbols[i].data_ptr(), outs[i].data_ptr(), scales[i].data_ptr(), symbols[i].numel()
            ck.it[j].beta = betas[i].data_ptr() if betas[i] is not None else None
        ck.n_items = m
        L.check(lib.bnerv_dequant_table(L.stream(), C.byref(ck)), "bnerv_dequant_table")
    return outs


class HuffDequant:
    """The device side of one qstream payload, ready to launch: the bit string (padded by two zero words), one
    descriptor per run (64-bit start bit, item, first element; built here from the u16 run lengths) and the item table.

        words      uint32 numpy array: the bit string as it lies in the file
        lengths    the 257 code lengths
        items      one (out, min, scale, red, inner, run_bits) per tensor: out a contiguous fp32 device tensor, min / scale contiguous fp32
                   or fp16 device tensors of out.numel() / red entries, run_bits its uint16 run lengths
    launch() decodes and de-quantises everything in one kernel; check() reads the device error word (a host sync) and raises ValueError
    when a run did not end on its recorded bit."""
    _name, _entry, _leaves = "huff_dequant", "bnerv_huff_dequant", L.HUFF_LEAVES
    _item_struct = L.HuffItem
    _item_dtype = [("out", "<u8"), ("min", "<u8"), ("scale", "<u8"), ("dtype", "<i4"), ("n", "<u4"), ("red", "<u4"), ("inner", "<u4")]

    def __init__(self, words, lengths, items, run=L.HUFF_RUN):
        import numpy as np
        if not items:
            raise ValueError(f"{self._name}: no items")
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.uint8)
        if self.lengths.size != self._leaves:
            raise ValueError(f"{self._name}: need {self._leaves} code lengths")
        if run != L.HUFF_RUN:
            raise ValueError(f"{self._name}: the kernel is built for runs of {L.HUFF_RUN} symbols, not {run}")
        self.run = int(run)
        table = np.zeros(len(items), dtype=self._item_dtype)
        assert table.dtype.itemsize == C.sizeof(self._item_struct)
        starts, item_of, first_of, bit = [], [], [], 0
        device = items[0][0].device
        for k, item in enumerate(items):
            table[k] = self._item(k, item, device)
            n, rb = int(table[k]["n"]), np.ascontiguousarray(item[-1], dtype=np.uint16)
            n_runs = (n + run - 1) // run
            if rb.size != n_runs:
                raise ValueError(f"{self._name}: item {k}: {rb.size} run lengths for {n_runs} runs")
            ends = bit + np.cumsum(rb, dtype=np.uint64)
            starts.append(np.concatenate([np.array([bit], dtype=np.uint64), ends[:-1]]))
            item_of.append(np.full(n_runs, k, dtype=np.uint32))
            first_of.append(np.arange(n_runs, dtype=np.uint32) * np.uint32(run))
            bit = int(ends[-1])
        if (bit + 31) // 32 != words.size:
            raise ValueError(f"{self._name}: the run lengths add up to {bit} bits, the bit string has {words.size} words")
        self.n_runs = int(sum(a.size for a in starts))
        runs = np.zeros(self.n_runs + 1, dtype=np.dtype([("start_bit", "<u8"), ("item", "<u4"), ("first", "<u4")]))
        assert runs.dtype.itemsize == C.sizeof(L.HuffRun)
        runs["start_bit"][:-1], runs["item"][:-1], runs["first"][:-1] = np.concatenate(starts), np.concatenate(item_of), np.concatenate(first_of)
        runs["start_bit"][-1] = bit                              # the sentinel: where the last run ends
        padded = np.zeros(words.size + 2, dtype=np.uint32)       # the kernel clamps every read to these words
        padded[:words.size] = words
        up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(device)      # noqa: E731
        self.words, self.runs, self.items = up(padded), up(runs), up(table)
        self.n_words, self.n_items = padded.size, len(items)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[:-1] for it in items]

    def _item(self, k, item, device):
        """The row of the item table for items[k], checked."""
        out, lo, step, red, inner, _ = item
        L.require_device(out, "out"), L.require_device(lo, "min"), L.require_device(step, "scale")
        n, red, inner = out.numel(), int(red), int(inner)
        if out.dtype != torch.float32 or not out.is_contiguous() or n == 0 or n >= 2 ** 31 or out.data_ptr() % 4 or out.device != device:
            raise ValueError(f"{self._name}: item {k}: out must be a non-empty contiguous 4-byte aligned fp32 tensor on {device} (below 2^31 elements)")
        if red < 1 or inner < 1 or n % (red * inner):
            raise ValueError(f"{self._name}: item {k}: {n} elements do not split into slices of red={red}, inner={inner}")
        slices = n // red
        if lo.dtype != step.dtype or lo.dtype not in (torch.float32, torch.float16) or lo.numel() != slices or step.numel() != slices \
                or not lo.is_contiguous() or not step.is_contiguous() or (lo.data_ptr() | step.data_ptr()) % lo.element_size():
            raise ValueError(f"{self._name}: item {k}: min and scale must be contiguous fp32 or fp16 tensors of {slices} entries each")
        return (out.data_ptr(), lo.data_ptr(), step.data_ptr(), L.HUFF_F16 if lo.dtype == torch.float16 else L.HUFF_F32, n, red, inner)

    def launch(self):
        L.check(getattr(L.load(), self._entry)(L.stream(), L.ptr(self.words), self.n_words, L.ptr(self.runs), self.n_runs, L.ptr(self.items), self.n_items,
                                               self.lengths.ctypes.data, self.run, L.ptr(self.err)), self._entry)
        return self

    def check(self):
        if int(self.err.item()) != 0:
            raise ValueError(f"{self._name}: a run of the bit string did not end on its recorded bit (the payload does not match its run index)")
        return self


def huff_dequant(words, lengths, items, run=L.HUFF_RUN):
    """Huffman-decode a qstream bit string and de-quantise it into the items' `out` tensors IN PLACE, one launch:
    out[i] = float(min[s]) + float(scale[s]) * float(q[i]), s = (i // (red * inner)) * inner + i % inner, product and sum one fp32
    operation each -- the `rebuilt` of hnerv_utils.quant_tensor, bit for bit.  Arguments: HuffDequant.  Raises ValueError when the device
    reports a run that did not end on its recorded bit."""
    HuffDequant(words, lengths, items, run).launch().check()
    return [it[0] for it in items]


class HuffzDequant(HuffDequant):
    """The device side of one zstream payload: HuffDequant under the 266-leaf code, launched as bnerv_huffz_dequant.
    A run is 256 ELEMENTS; zero elements are written as +0.0.  check() raises ValueError when a run did not end on its recorded bit, met
    the EOF leaf, or held a zero-run leaf that passed its element count."""
    _name, _entry, _leaves = "huffz_dequant", "bnerv_huffz_dequant", L.HUFFZ_LEAVES


def huffz_dequant(words, lengths, items, run=L.HUFF_RUN):
    """Huffman-decode a zstream bit string and de-quantise it into the items' `out` tensors IN PLACE, one launch:
    out[i] = keep[i] ? float(min[s]) + float(scale[s]) * float(q[i]) : +0.0 -- the `rebuilt` of hnerv_utils.quant_tensor_sparse, bit for
    bit.  Arguments: HuffDequant, with 266 code lengths.  Raises ValueError when the device reports a run that did not decode to its
    element count on its recorded bit."""
    HuffzDequant(words, lengths, items, run).launch().check()
    return [it[0] for it in items]


class AnsDequant:
    """The device side of one chunked CEM payload (rstream.py), ready to launch: the words of all runs (padded by two
    zero words), the first word of every run, one cumulative table per record (built on the host by bnerv_ans_gaussian_cdf, all uploaded as
    one array), the item table and the block table -- a block serves up to 64 consecutive runs of one record.

        words      uint32 numpy array: the runs of all items back to back, as they lie in the file
        items      one (out, scale, lo, hi, mean, std, run_words, beta) per record: out a contiguous fp32 device tensor (any 4-byte alignment),
                   scale / mean / std floats, [lo, hi] the symbol range (at most 4096 symbols), run_words the uint16 word count of every run,
                   beta a float or None
        run        symbols per run: a multiple of 64 in 64..4096
    Every run's span is validated against the words here, before anything is uploaded.  launch() decodes and de-quantises everything in one
    kernel; check() reads the device error word (a host sync) and raises ValueError when a run did not consume exactly its words or did not
    end with an empty state."""

    def __init__(self, words, items, run):
        import numpy as np
        from .lib.entropy_model import ans_gaussian_cdf
        if not items:
            raise ValueError("ans_dequant: no items")
        run = int(run)
        if not L.RANS_MIN_RUN <= run <= L.RANS_MAX_RUN or run % 64:
            raise ValueError(f"ans_dequant: run = {run} (a multiple of 64 in {L.RANS_MIN_RUN}..{L.RANS_MAX_RUN})")
        self.run = run
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        table = np.zeros(len(items), dtype=np.dtype([("out", "<u8"), ("scale", "<f4"), ("beta", "<f4"), ("lo", "<i4"), ("n", "<u4"), ("table", "<u4"),
                                                     ("alphabet", "<u4"), ("has_beta", "<i4"), ("_pad", "<i4")]))
        assert table.dtype.itemsize == C.sizeof(L.RansItem)
        device = items[0][0].device
        cdfs, lengths, blocks, at_table, at_run = [], [], [], 0, 0
        for k, (out, scale, lo, hi, mean, std, run_words, beta) in enumerate(items):
            L.require_device(out, "out")
            n, lo, hi = out.numel(), int(lo), int(hi)
            if out.dtype != torch.float32 or not out.is_contiguous() or n == 0 or n >= 2 ** 31 or out.data_ptr() % 4 or out.device != device:
                raise ValueError(f"ans_dequant: item {k}: out must be a non-empty contiguous 4-byte aligned fp32 tensor on {device} (below 2^31 elements)")
            if not 2 <= hi - lo + 1 <= L.RANS_MAX_ALPHABET:
                raise ValueError(f"ans_dequant: item {k}: the symbol range [{lo}, {hi}] has {hi - lo + 1} symbols (2..{L.RANS_MAX_ALPHABET})")
            rw = np.ascontiguousarray(run_words, dtype=np.uint16).reshape(-1)
            n_runs = (n + run - 1) // run
            if rw.size != n_runs:
                raise ValueError(f"ans_dequant: item {k}: {rw.size} run lengths for {n_runs} runs")
            if int(rw.min()) < 2:
                raise ValueError(f"ans_dequant: item {k}: run {int(rw.argmin())} has {int(rw.min())} words, fewer than its two state words")
            cdf = ans_gaussian_cdf(lo, hi, mean, std)
            table[k] = (out.data_ptr(), np.float32(scale), np.float32(0.0 if beta is None else beta), lo, n, at_table, cdf.size - 1, int(beta is not None), 0)
            cdfs.append(cdf)
            at_table += cdf.size
            lengths.append(rw)
            first = np.arange(0, n_runs, 64, dtype=np.uint32)
            blk = np.zeros((first.size, 4), dtype=np.uint32)
            blk[:, 0], blk[:, 1], blk[:, 2] = k, at_run + first, first
            blocks.append(blk)
            at_run += n_runs
        lengths = np.concatenate(lengths)
        starts = np.zeros(lengths.size + 1, dtype=np.uint64)
        np.cumsum(lengths, dtype=np.uint64, out=starts[1:])
        if int(starts[-1]) != words.size or words.size + 2 >= 2 ** 32:
            raise ValueError(f"ans_dequant: the run lengths add up to {int(starts[-1])} words, the payload has {words.size}")
        padded = np.zeros(words.size + 2, dtype=np.uint32)       # (every run's span ends at or before words.size: validated just above)
        padded[:words.size] = words
        blocks = np.concatenate(blocks)
        assert blocks.dtype.itemsize * 4 == C.sizeof(L.RansBlock)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)      # noqa: E731
        self.words, self.starts, self.blocks, self.items, self.tables = up(padded), up(starts.astype(np.uint32)), up(blocks), up(table), up(np.concatenate(cdfs))
        self.n_words, self.n_runs, self.n_blocks, self.n_items, self.n_table_words = padded.size, int(lengths.size), int(blocks.shape[0]), len(items), at_table
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self):
        L.check(L.load().bnerv_rans_dequant(L.stream(), L.ptr(self.words), self.n_words, L.ptr(self.starts), self.n_runs, L.ptr(self.blocks), self.n_blocks,
                                            L.ptr(self.items), self.n_items, L.ptr(self.tables), self.n_table_words, self.run, L.ptr(self.err)), "bnerv_rans_dequant")
        return self

    def check(self):
        e = int(self.err.item())
        if e != 0:
            raise ValueError("ans_dequant: " + ("a descriptor points outside the uploaded arrays" if e & 2 else
                                                "a run did not consume exactly its words and end with an empty state (the payload does not match its run index)"))
        return self


def ans_dequant(words, items, run):
    """Range-ANS-decode the runs of a chunked CEM payload and de-quantise them into the items' `out` tensors IN PLACE, one launch:
    out[i] = float(symbol) * scale (+ beta), product and sum one fp32 operation each -- Scale_T's and ScaleBeta_T's expressions, bit for bit.
    Arguments: AnsDequant.  Raises ValueError when the device reports a run that did not decode."""
    AnsDequant(words, items, run).launch().check()
    return [it[0] for it in items]


class AnsDequantTables(AnsDequant):
    """AnsDequant for a chunked CEM payload whose records bring their tables (estream.py): the same uploads, the same
    kernel (bnerv_rans_dequant), launch() and check(), with every record's cumulative table given by the caller instead of built from
    (mean, std).

        items      one (out, scale, lo, cdf, run_words, beta) per record: cdf the record's cumulative table (uint32 numpy, A + 1 entries rising
                   strictly from 0 to 2^24, 2 <= A <= 4096: symbol lo + i owns [cdf[i], cdf[i + 1])); the rest as in AnsDequant"""

    def __init__(self, words, items, run):
        import numpy as np
        if not items:
            raise ValueError("ans_dequant_tables: no items")
        run = int(run)
        if not L.RANS_MIN_RUN <= run <= L.RANS_MAX_RUN or run % 64:
            raise ValueError(f"ans_dequant_tables: run = {run} (a multiple of 64 in {L.RANS_MIN_RUN}..{L.RANS_MAX_RUN})")
        self.run = run
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        table = np.zeros(len(items), dtype=np.dtype([("out", "<u8"), ("scale", "<f4"), ("beta", "<f4"), ("lo", "<i4"), ("n", "<u4"), ("table", "<u4"),
                                                     ("alphabet", "<u4"), ("has_beta", "<i4"), ("_pad", "<i4")]))
        assert table.dtype.itemsize == C.sizeof(L.RansItem)
        device = items[0][0].device
        cdfs, lengths, blocks, at_table, at_run = [], [], [], 0, 0
        for k, (out, scale, lo, cdf, run_words, beta) in enumerate(items):
            L.require_device(out, "out")
            n = out.numel()
            if out.dtype != torch.float32 or not out.is_contiguous() or n == 0 or n >= 2 ** 31 or out.data_ptr() % 4 or out.device != device:
                raise ValueError(f"ans_dequant_tables: item {k}: out must be a non-empty contiguous 4-byte aligned fp32 tensor on {device} (below 2^31 elements)")
            cdf = np.ascontiguousarray(cdf, dtype=np.uint32).reshape(-1)
            if not 2 <= cdf.size - 1 <= L.RANS_MAX_ALPHABET:
                raise ValueError(f"ans_dequant_tables: item {k}: a table of {cdf.size - 1} symbols (2..{L.RANS_MAX_ALPHABET})")
            if cdf[0] != 0 or cdf[-1] != 1 << 24 or (np.diff(cdf.astype(np.int64)) <= 0).any():
                raise ValueError(f"ans_dequant_tables: item {k}: the cumulative table does not rise strictly from 0 to 2^24")
            rw = np.ascontiguousarray(run_words, dtype=np.uint16).reshape(-1)
            n_runs = (n + run - 1) // run
            if rw.size != n_runs:
                raise ValueError(f"ans_dequant_tables: item {k}: {rw.size} run lengths for {n_runs} runs")
            if int(rw.min()) < 2:
                raise ValueError(f"ans_dequant_tables: item {k}: run {int(rw.argmin())} has {int(rw.min())} words, fewer than its two state words")
            table[k] = (out.data_ptr(), np.float32(scale), np.float32(0.0 if beta is None else beta), int(lo), n, at_table, cdf.size - 1, int(beta is not None), 0)
            cdfs.append(cdf)
            at_table += cdf.size
            lengths.append(rw)
            first = np.arange(0, n_runs, 64, dtype=np.uint32)
            blk = np.zeros((first.size, 4), dtype=np.uint32)
            blk[:, 0], blk[:, 1], blk[:, 2] = k, at_run + first, first
            blocks.append(blk)
            at_run += n_runs
        lengths = np.concatenate(lengths)
        starts = np.zeros(lengths.size + 1, dtype=np.uint64)
        np.cumsum(lengths, dtype=np.uint64, out=starts[1:])
        if int(starts[-1]) != words.size or words.size + 2 >= 2 ** 32:
            raise ValueError(f"ans_dequant_tables: the run lengths add up to {int(starts[-1])} words, the payload has {words.size}")
        padded = np.zeros(words.size + 2, dtype=np.uint32)       # (every run's span ends at or before words.size: validated just above)
        padded[:words.size] = words
        blocks = np.concatenate(blocks)
        self.words, self.starts, self.blocks, self.items, self.tables = (_upload(a, device) for a in (padded, starts.astype(np.uint32), blocks, table, np.concatenate(cdfs)))
        self.n_words, self.n_runs, self.n_blocks, self.n_items, self.n_table_words = padded.size, int(lengths.size), int(blocks.shape[0]), len(items), at_table
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]


def ans_dequant_tables(words, items, run):
    """ans_dequant with an explicit cumulative table per record.  Arguments: AnsDequantTables."""
    AnsDequantTables(words, items, run).launch().check()
    return [it[0] for it in items]


# ----------------------------------------------------------------------------------------------------------------------
# device encoder of the chunked CEM file with per-record tables (codec.encode(..., tables="empirical"); csrc/ransenc.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _symbol_items(items, what):
    """Validates (symbols, lo, ...) items: non-empty contiguous int32 device tensors below 2^31 elements, all on one device."""
    device = items[0][0].device
    for k, it in enumerate(items):
        sym = L.require_device(it[0], "symbols")
        if sym.dtype != torch.int32 or not sym.is_contiguous() or sym.numel() == 0 or sym.numel() >= 2 ** 31 or sym.data_ptr() % 4 or sym.device != device:
            raise ValueError(f"{what}: item {k}: symbols must be a non-empty contiguous int32 tensor on {device} (below 2^31 elements)")
    return device


def _upload(a, device):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)


class SymHist:
    """The histograms of int32 symbol tensors, ONE launch (bnerv_sym_hist).

        items      one (symbols, lo, alphabet) per record: symbols a contiguous int32 device tensor (any 4-byte alignment), counted on
                   [lo, lo + alphabet), alphabet in 1..4096
    launch() zeroes and fills `counts` (int32 device tensor, the records' histograms back to back; record k at offsets[k]); check() reads
    the device error word (a host sync) and raises ValueError when a symbol lay outside its record's range; host() is the list of the
    records' uint32 numpy histograms (one copy, after check())."""

    def __init__(self, items):
        import numpy as np
        if not items:
            raise ValueError("sym_hist: no items")
        device = _symbol_items(items, "sym_hist")
        table = np.zeros(len(items), dtype=np.dtype([("sym", "<u8"), ("n", "<u4"), ("lo", "<i4"), ("alphabet", "<u4"), ("out", "<u4")]))
        assert table.dtype.itemsize == C.sizeof(L.HistItem)
        blocks, self.offsets, at = [], [], 0
        for k, (sym, lo, alphabet) in enumerate(items):
            alphabet = int(alphabet)
            if not 1 <= alphabet <= L.RANS_MAX_ALPHABET:
                raise ValueError(f"sym_hist: item {k}: an alphabet of {alphabet} symbols (1..{L.RANS_MAX_ALPHABET})")
            table[k] = (sym.data_ptr(), sym.numel(), int(lo), alphabet, at)
            first = np.arange(0, sym.numel(), L.HIST_SLICE, dtype=np.uint32)
            blocks.append(np.stack([np.full(first.size, k, dtype=np.uint32), first], axis=1))
            self.offsets.append(at)
            at += alphabet
        blocks = np.concatenate(blocks)
        self.alphabets = [int(it[2]) for it in items]
        self.items, self.blocks = _upload(table, device), _upload(blocks, device)
        self.n_items, self.n_blocks, self.n_counts = len(items), int(blocks.shape[0]), at
        self.counts = torch.zeros(at, dtype=torch.int32, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self, zero=True):
        """zero=False adds to the counts that are there (a caller that has just zeroed them; the kernel alone under a timer)."""
        if zero:
            self.counts.zero_()
        L.check(L.load().bnerv_sym_hist(L.stream(), L.ptr(self.items), self.n_items, L.ptr(self.blocks), self.n_blocks, L.ptr(self.counts), self.n_counts,
                                        L.ptr(self.err)), "bnerv_sym_hist")
        return self

    def check(self):
        e = int(self.err.item())
        if e != 0:
            raise ValueError("sym_hist: " + ("a descriptor points outside the uploaded arrays" if e & 2 else "a symbol lies outside its record's range"))
        return self

    def host(self):
        import numpy as np
        flat = self.counts.cpu().numpy().view(np.uint32)
        return [flat[o:o + a].copy() for o, a in zip(self.offsets, self.alphabets)]


def sym_hist(items):
    """The uint32 numpy histogram of every item, one launch.  Arguments: SymHist.  Raises ValueError for a symbol outside its range."""
    return SymHist(items).launch().check().host()


class AnsEncodeRuns:
    """The device encoder of range-ANS runs (bnerv_rans_encode, bnerv_rans_compact), the inverse of AnsDequantTables.

        items      one (symbols, lo, cdf) per message: symbols a contiguous int32 device tensor (any 4-byte alignment; items may share one),
                   cdf its cumulative table (uint32 numpy, A + 1 entries rising strictly from 0 to 2^24, 2 <= A <= 4096)
        run        symbols per run: a multiple of 64 in 64..4096
    launch() encodes every run of every item in ONE kernel, each into a slot of its own (run * 24 / 32 + 3 words, the host coder's bound);
    check() reads the device error word (a host sync) and raises ValueError when a symbol lay outside its table.  run_words() is the
    uint16 word count of every run per item (one copy); result(chosen) -- the items to keep, in output order; default all -- compacts their
    runs in ONE more launch and returns (uint32 numpy words back to back, [run_words of each chosen item]): bit for bit what
    lib.entropy_model.ans_encode_table_runs returns item by item."""

    def __init__(self, items, run):
        import numpy as np
        if not items:
            raise ValueError("ans_encode_runs: no items")
        run = int(run)
        if not L.RANS_MIN_RUN <= run <= L.RANS_MAX_RUN or run % 64:
            raise ValueError(f"ans_encode_runs: run = {run} (a multiple of 64 in {L.RANS_MIN_RUN}..{L.RANS_MAX_RUN})")
        self.run, self.slot_words = run, run * 24 // 32 + 3
        self.device = device = _symbol_items(items, "ans_encode_runs")
        table = np.zeros(len(items), dtype=np.dtype([("sym", "<u8"), ("n", "<u4"), ("lo", "<i4"), ("alphabet", "<u4"), ("table", "<u4")]))
        assert table.dtype.itemsize == C.sizeof(L.RencItem)
        cdfs, blocks, self.first_run, at_table, at_run = [], [], [], 0, 0
        for k, (sym, lo, cdf) in enumerate(items):
            cdf = np.ascontiguousarray(cdf, dtype=np.uint32).reshape(-1)
            if not 2 <= cdf.size - 1 <= L.RANS_MAX_ALPHABET:
                raise ValueError(f"ans_encode_runs: item {k}: a table of {cdf.size - 1} symbols (2..{L.RANS_MAX_ALPHABET})")
            if cdf[0] != 0 or cdf[-1] != 1 << 24 or (np.diff(cdf.astype(np.int64)) <= 0).any():
                raise ValueError(f"ans_encode_runs: item {k}: the cumulative table does not rise strictly from 0 to 2^24")
            n_runs = (sym.numel() + run - 1) // run
            table[k] = (sym.data_ptr(), sym.numel(), int(lo), cdf.size - 1, at_table)
            cdfs.append(cdf)
            at_table += cdf.size
            first = np.arange(0, n_runs, 64, dtype=np.uint32)
            blk = np.zeros((first.size, 4), dtype=np.uint32)
            blk[:, 0], blk[:, 1], blk[:, 2] = k, at_run + first, first
            blocks.append(blk)
            self.first_run.append(at_run)
            at_run += n_runs
        self.first_run.append(at_run)
        blocks = np.concatenate(blocks)
        if at_run * self.slot_words >= 2 ** 32:
            raise ValueError(f"ans_encode_runs: {at_run} runs of {run} symbols need more than 2^32 scratch words")
        self.items, self.blocks, self.tables = _upload(table, device), _upload(blocks, device), _upload(np.concatenate(cdfs), device)
        self.n_items, self.n_blocks, self.n_table_words, self.n_slots = len(items), int(blocks.shape[0]), at_table, at_run
        self.slots = torch.empty(at_run * self.slot_words, dtype=torch.int32, device=device)
        self.counts = torch.zeros(at_run, dtype=torch.int16, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self):
        L.check(L.load().bnerv_rans_encode(L.stream(), L.ptr(self.blocks), self.n_blocks, L.ptr(self.items), self.n_items, L.ptr(self.tables), self.n_table_words,
                                           self.run, L.ptr(self.slots), self.n_slots, L.ptr(self.counts), L.ptr(self.err)), "bnerv_rans_encode")
        return self

    def check(self):
        e = int(self.err.item())
        if e != 0:
            raise ValueError("ans_encode_runs: " + ("a descriptor points outside the uploaded arrays" if e & 2 else
                                                    "a symbol lies outside its table (or a run outgrew its slot)"))
        return self

    def run_words(self):
        import numpy as np
        flat = self.counts.cpu().numpy().view(np.uint16)
        return [flat[a:b].copy() for a, b in zip(self.first_run[:-1], self.first_run[1:])]

    def compact(self, chosen, run_words):
        """An AnsCompact that gathers the runs of the items `chosen`, in that order; run_words: what run_words() returned."""
        return AnsCompact(self, chosen, run_words)

    def result(self, chosen=None):
        self.check()
        chosen = list(range(self.n_items)) if chosen is None else list(chosen)
        rw = self.run_words()
        job = self.compact(chosen, rw).launch().check()
        return job.host(), [rw[k] for k in chosen]


class AnsCompact:
    """The runs of the chosen items of an AnsEncodeRuns, copied from their slots to one array back to back (bnerv_rans_compact): the
    destination of every run is the exclusive sum of the word counts before it.  launch(), check() as elsewhere; `words`: the int32 device
    tensor; host(): its uint32 numpy copy."""

    def __init__(self, enc, chosen, run_words):
        import numpy as np
        if not chosen:
            raise ValueError("ans_compact: no items")
        counts = np.concatenate([run_words[k] for k in chosen]).astype(np.uint32)
        slot = np.concatenate([np.arange(enc.first_run[k], enc.first_run[k + 1], dtype=np.uint32) for k in chosen])
        ends = np.cumsum(counts, dtype=np.uint64)
        if int(counts.min()) < 2 or int(counts.max()) > enc.slot_words or int(ends[-1]) >= 2 ** 32:
            raise ValueError(f"ans_compact: run word counts in {int(counts.min())}..{int(counts.max())} (2..{enc.slot_words}; was the encoder checked?)")
        copies = np.zeros((counts.size, 4), dtype=np.uint32)
        copies[:, 0], copies[:, 1], copies[:, 2] = slot, (ends - counts).astype(np.uint32), counts
        assert copies.dtype.itemsize * 4 == C.sizeof(L.RansCopy)
        self.enc, self.n_copies, self.n_out = enc, int(counts.size), int(ends[-1])
        self.copies = _upload(copies, enc.device)
        self.words = torch.empty(self.n_out, dtype=torch.int32, device=enc.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=enc.device)

    def launch(self):
        e = self.enc
        L.check(L.load().bnerv_rans_compact(L.stream(), L.ptr(e.slots), e.n_slots, e.slot_words, L.ptr(self.copies), self.n_copies, L.ptr(self.words), self.n_out,
                                            L.ptr(self.err)), "bnerv_rans_compact")
        return self

    def check(self):
        if int(self.err.item()) != 0:
            raise ValueError("ans_compact: a copy points outside the slots or the output")
        return self

    def host(self):
        import numpy as np
        return self.words.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# records that span more than 4096 symbol values (wstream.py, codec.encode(..., wide=True); csrc/ransw.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _wide_shape(what, k, lo, hi, shift, cdf=None):
    """Validates the (range, shift, table) of a wide item -> (lo, hi, shift, B, cdf): B = ceil((hi - lo + 1) / 2^shift) buckets, 2..4096,
    and, where a table is given, its B + 1 entries rising strictly from 0 to 2^24."""
    import numpy as np
    lo, hi, shift = int(lo), int(hi), int(shift)
    if not 0 <= shift <= L.RANSW_MAX_SHIFT:
        raise ValueError(f"{what}: item {k}: shift = {shift} (0..{L.RANSW_MAX_SHIFT})")
    B = (hi - lo + (1 << shift)) >> shift
    if hi < lo or hi - lo >= 1 << 28 or not 2 <= B <= L.RANS_MAX_ALPHABET:
        raise ValueError(f"{what}: item {k}: the range [{lo}, {hi}] at shift {shift} has {B} buckets (2..{L.RANS_MAX_ALPHABET})")
    if cdf is not None:
        cdf = np.ascontiguousarray(cdf, dtype=np.uint32).reshape(-1)
        if cdf.size - 1 != B:
            raise ValueError(f"{what}: item {k}: a table of {cdf.size - 1} buckets for the {B} of [{lo}, {hi}] at shift {shift}")
        if cdf[0] != 0 or cdf[-1] != 1 << 24 or (np.diff(cdf.astype(np.int64)) <= 0).any():
            raise ValueError(f"{what}: item {k}: the cumulative table does not rise strictly from 0 to 2^24")
    return lo, hi, shift, B, cdf


_WSYM_DTYPE = [("sym", "<u8"), ("n", "<u4"), ("lo", "<i4"), ("alphabet", "<u4"), ("at", "<u4"), ("shift", "<u4"), ("span_m1", "<u4")]


class SymHistWide(SymHist):
    """SymHist over buckets, ONE launch (bnerv_sym_hist_wide): counts of (symbol - lo) >> shift.

        items      one (symbols, lo, hi, shift) per record: symbols a contiguous int32 device tensor (any 4-byte alignment), counted on
                   [lo, hi] in ceil((hi - lo + 1) / 2^shift) buckets (2..4096), shift in 0..16
    launch(), check(), host() as SymHist's."""

    def __init__(self, items):
        import numpy as np
        if not items:
            raise ValueError("sym_hist_wide: no items")
        device = _symbol_items(items, "sym_hist_wide")
        table = np.zeros(len(items), dtype=np.dtype(_WSYM_DTYPE))
        assert table.dtype.itemsize == C.sizeof(L.WsymItem)
        blocks, self.offsets, self.alphabets, at = [], [], [], 0
        for k, (sym, lo, hi, shift) in enumerate(items):
            lo, hi, shift, B, _ = _wide_shape("sym_hist_wide", k, lo, hi, shift)
            table[k] = (sym.data_ptr(), sym.numel(), lo, B, at, shift, hi - lo)
            first = np.arange(0, sym.numel(), L.HIST_SLICE, dtype=np.uint32)
            blocks.append(np.stack([np.full(first.size, k, dtype=np.uint32), first], axis=1))
            self.offsets.append(at)
            self.alphabets.append(B)
            at += B
        blocks = np.concatenate(blocks)
        self.items, self.blocks = _upload(table, device), _upload(blocks, device)
        self.n_items, self.n_blocks, self.n_counts = len(items), int(blocks.shape[0]), at
        self.counts = torch.zeros(at, dtype=torch.int32, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self, zero=True):
        if zero:
            self.counts.zero_()
        L.check(L.load().bnerv_sym_hist_wide(L.stream(), L.ptr(self.items), self.n_items, L.ptr(self.blocks), self.n_blocks, L.ptr(self.counts), self.n_counts,
                                             L.ptr(self.err)), "bnerv_sym_hist_wide")
        return self


def sym_hist_wide(items):
    """The uint32 numpy bucket histogram of every item, one launch.  Arguments: SymHistWide.  Raises ValueError for a symbol outside its range."""
    return SymHistWide(items).launch().check().host()


class AnsEncodeRunsWide(AnsEncodeRuns):
    """AnsEncodeRuns for ranges of any width (bnerv_rans_encode_wide, bnerv_rans_compact), the inverse of AnsDequantWide.

        items      one (symbols, lo, hi, cdf, shift) per message: symbols a contiguous int32 device tensor in [lo, hi] (any 4-byte alignment; items
                   may share one), cdf the cumulative table of its B = ceil((hi - lo + 1) / 2^shift) buckets (uint32 numpy, B + 1 entries
                   rising strictly from 0 to 2^24, 2 <= B <= 4096), shift in 0..16
        run        symbols per run: a multiple of 64 in 64..4096
    A run of an item may take run * (24 + shift) / 32 + 3 words, the host coder's bound; the slots of one launch are as far apart as the
    largest shift needs.  launch(), check(), run_words(), compact(), result() as AnsEncodeRuns's: bit for bit what
    lib.entropy_model.ans_encode_wide_runs returns item by item."""

    def __init__(self, items, run):
        import numpy as np
        if not items:
            raise ValueError("ans_encode_runs_wide: no items")
        run = int(run)
        if not L.RANS_MIN_RUN <= run <= L.RANS_MAX_RUN or run % 64:
            raise ValueError(f"ans_encode_runs_wide: run = {run} (a multiple of 64 in {L.RANS_MIN_RUN}..{L.RANS_MAX_RUN})")
        self.run = run
        self.device = device = _symbol_items(items, "ans_encode_runs_wide")
        table = np.zeros(len(items), dtype=np.dtype(_WSYM_DTYPE))
        assert table.dtype.itemsize == C.sizeof(L.WsymItem)
        cdfs, blocks, self.first_run, at_table, at_run, top = [], [], [], 0, 0, 0
        for k, (sym, lo, hi, cdf, shift) in enumerate(items):
            lo, hi, shift, B, cdf = _wide_shape("ans_encode_runs_wide", k, lo, hi, shift, cdf)
            n_runs = (sym.numel() + run - 1) // run
            table[k] = (sym.data_ptr(), sym.numel(), lo, B, at_table, shift, hi - lo)
            cdfs.append(cdf)
            at_table += cdf.size
            top = max(top, shift)
            first = np.arange(0, n_runs, 64, dtype=np.uint32)
            blk = np.zeros((first.size, 4), dtype=np.uint32)
            blk[:, 0], blk[:, 1], blk[:, 2] = k, at_run + first, first
            blocks.append(blk)
            self.first_run.append(at_run)
            at_run += n_runs
        self.first_run.append(at_run)
        self.slot_words = run * (24 + top) // 32 + 3
        blocks = np.concatenate(blocks)
        if at_run * self.slot_words >= 2 ** 32:
            raise ValueError(f"ans_encode_runs_wide: {at_run} runs of {run} symbols need more than 2^32 scratch words")
        self.items, self.blocks, self.tables = _upload(table, device), _upload(blocks, device), _upload(np.concatenate(cdfs), device)
        self.n_items, self.n_blocks, self.n_table_words, self.n_slots = len(items), int(blocks.shape[0]), at_table, at_run
        self.slots = torch.empty(at_run * self.slot_words, dtype=torch.int32, device=device)
        self.counts = torch.zeros(at_run, dtype=torch.int16, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self):
        L.check(L.load().bnerv_rans_encode_wide(L.stream(), L.ptr(self.blocks), self.n_blocks, L.ptr(self.items), self.n_items, L.ptr(self.tables),
                                                self.n_table_words, self.run, L.ptr(self.slots), self.n_slots, self.slot_words, L.ptr(self.counts),
                                                L.ptr(self.err)), "bnerv_rans_encode_wide")
        return self

    def check(self):
        e = int(self.err.item())
        if e != 0:
            raise ValueError("ans_encode_runs_wide: " + ("a descriptor points outside the uploaded arrays" if e & 2 else
                                                         "a symbol lies outside its range (or a run outgrew its slot)"))
        return self


class AnsDequantWide(AnsDequant):
    """AnsDequantTables for records of any width (wstream.py): the same uploads, launch() and check(), with the kernel
    that pops `shift` raw bits after every bucket (bnerv_rans_dequant_wide).

        items      one (out, scale, lo, hi, cdf, shift, run_words, beta) per record: [lo, hi] the symbol range, cdf the cumulative table of its
                   B = ceil((hi - lo + 1) / 2^shift) buckets (uint32 numpy, B + 1 entries rising strictly from 0 to 2^24, 2 <= B <= 4096),
                   shift in 0..16; the rest as in AnsDequant"""
    _out_dtype, _out_name = torch.float32, "fp32"

    def __init__(self, words, items, run):
        import numpy as np
        if not items:
            raise ValueError("ans_dequant_wide: no items")
        run = int(run)
        if not L.RANS_MIN_RUN <= run <= L.RANS_MAX_RUN or run % 64:
            raise ValueError(f"ans_dequant_wide: run = {run} (a multiple of 64 in {L.RANS_MIN_RUN}..{L.RANS_MAX_RUN})")
        self.run = run
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        table = np.zeros(len(items), dtype=np.dtype([("out", "<u8"), ("scale", "<f4"), ("beta", "<f4"), ("lo", "<i4"), ("n", "<u4"), ("table", "<u4"),
                                                     ("alphabet", "<u4"), ("has_beta", "<i4"), ("shift", "<u4"), ("span_m1", "<u4"), ("_pad", "<u4")]))
        assert table.dtype.itemsize == C.sizeof(L.RanswItem)
        device = items[0][0].device
        cdfs, lengths, blocks, at_table, at_run = [], [], [], 0, 0
        for k, (out, scale, lo, hi, cdf, shift, run_words, beta) in enumerate(items):
            L.require_device(out, "out")
            n = out.numel()
            if out.dtype != self._out_dtype or not out.is_contiguous() or n == 0 or n >= 2 ** 31 or out.data_ptr() % 4 or out.device != device:
                raise ValueError(f"ans_dequant_wide: item {k}: out must be a non-empty contiguous 4-byte aligned {self._out_name} tensor on {device} (below 2^31 elements)")
            lo, hi, shift, B, cdf = _wide_shape("ans_dequant_wide", k, lo, hi, shift, cdf)
            rw = np.ascontiguousarray(run_words, dtype=np.uint16).reshape(-1)
            n_runs = (n + run - 1) // run
            if rw.size != n_runs:
                raise ValueError(f"ans_dequant_wide: item {k}: {rw.size} run lengths for {n_runs} runs")
            if int(rw.min()) < 2:
                raise ValueError(f"ans_dequant_wide: item {k}: run {int(rw.argmin())} has {int(rw.min())} words, fewer than its two state words")
            table[k] = (out.data_ptr(), np.float32(scale), np.float32(0.0 if beta is None else beta), lo, n, at_table, B, int(beta is not None), shift, hi - lo, 0)
            cdfs.append(cdf)
            at_table += cdf.size
            lengths.append(rw)
            first = np.arange(0, n_runs, 64, dtype=np.uint32)
            blk = np.zeros((first.size, 4), dtype=np.uint32)
            blk[:, 0], blk[:, 1], blk[:, 2] = k, at_run + first, first
            blocks.append(blk)
            at_run += n_runs
        lengths = np.concatenate(lengths)
        starts = np.zeros(lengths.size + 1, dtype=np.uint64)
        np.cumsum(lengths, dtype=np.uint64, out=starts[1:])
        if int(starts[-1]) != words.size or words.size + 2 >= 2 ** 32:
            raise ValueError(f"ans_dequant_wide: the run lengths add up to {int(starts[-1])} words, the payload has {words.size}")
        padded = np.zeros(words.size + 2, dtype=np.uint32)       # (every run's span ends at or before words.size: validated just above)
        padded[:words.size] = words
        blocks = np.concatenate(blocks)
        self.words, self.starts, self.blocks, self.items, self.tables = (_upload(a, device) for a in (padded, starts.astype(np.uint32), blocks, table, np.concatenate(cdfs)))
        self.n_words, self.n_runs, self.n_blocks, self.n_items, self.n_table_words = padded.size, int(lengths.size), int(blocks.shape[0]), len(items), at_table
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep = [it[0] for it in items]

    def launch(self):
        L.check(L.load().bnerv_rans_dequant_wide(L.stream(), L.ptr(self.words), self.n_words, L.ptr(self.starts), self.n_runs, L.ptr(self.blocks), self.n_blocks,
                                                 L.ptr(self.items), self.n_items, L.ptr(self.tables), self.n_table_words, self.run, L.ptr(self.err)),
                "bnerv_rans_dequant_wide")
        return self

    def check(self):
        e = int(self.err.item())
        if e != 0:
            raise ValueError("ans_dequant_wide: " + ("a descriptor points outside the uploaded arrays" if e & 2 else
                                                     "a run did not consume exactly its words and end with an empty state, or decoded a value past its range "
                                                     "(the payload does not match its run index)"))
        return self


def ans_dequant_wide(words, items, run):
    """ans_dequant_tables for records of any width.  Arguments: AnsDequantWide."""
    AnsDequantWide(words, items, run).launch().check()
    return [it[0] for it in items]


# ----------------------------------------------------------------------------------------------------------------------
# inter-coded frame embeddings (tstream.py, codec.encode(..., temporal=True); csrc/ranst.hip)
# ----------------------------------------------------------------------------------------------------------------------
class AnsDecodeWide(AnsDequantWide):
    """AnsDequantWide with an int32 result (bnerv_rans_decode_wide, the same kernel body): out[i] = lo + offset, the symbols a record holds.

        items      one (out, lo, hi, cdf, shift, run_words) per record: out a contiguous int32 device tensor; the rest as in AnsDequantWide"""
    _out_dtype, _out_name = torch.int32, "int32"

    def __init__(self, words, items, run):
        super().__init__(words, [(out, 1.0, lo, hi, cdf, shift, rw, None) for out, lo, hi, cdf, shift, rw in items], run)

    def launch(self):
        L.check(L.load().bnerv_rans_decode_wide(L.stream(), L.ptr(self.words), self.n_words, L.ptr(self.starts), self.n_runs, L.ptr(self.blocks), self.n_blocks,
                                                L.ptr(self.items), self.n_items, L.ptr(self.tables), self.n_table_words, self.run, L.ptr(self.err)),
                "bnerv_rans_decode_wide")
        return self


def _rows(t, name, dtype, what):
    """(N, P, pitch) of a 2-D device tensor whose rows are dense (stride 1 along p, any row pitch >= P), any 4-byte alignment."""
    L.require_device(t, name)
    if t.dim() != 2 or t.dtype != dtype or t.numel() == 0 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or t.data_ptr() % 4:
        raise ValueError(f"{what}: {name} must be a non-empty [N, P] {dtype} device tensor with dense rows (row pitch >= P), got {t.dtype} {tuple(t.shape)} "
                         f"strides {tuple(t.stride())}")
    return int(t.shape[0]), int(t.shape[1]), int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


class EmbedDelta:
    """The frame-to-frame differences of the embedding symbols and their statistics, ONE launch (bnerv_embed_delta).

        q          int32 [N, P] device tensor, dense rows at any row pitch and any 4-byte alignment
        d          None, or the int32 [N, P] tensor to write (same rules); row 0 is not written
    launch() zeroes the statistics and fills d[t] = q[t] - q[t - 1] for t >= 1; check() is there for the shape of the other ops (the kernel
    takes no index from a descriptor: nothing can be flagged); host() -> (lo, hi, s1, s2), numpy arrays of N entries (entry 0 is zero):
    min d and max d as int64, s1 = sum d as int64, s2 = sum d^2 mod 2^64 as uint64 -- one copy."""

    def __init__(self, q, d=None):
        self.N, self.P, self.q_pitch = _rows(q, "q", torch.int32, "embed_delta")
        if d is None:
            d = torch.empty(self.N, self.P, dtype=torch.int32, device=q.device)
        N, P, self.d_pitch = _rows(d, "d", torch.int32, "embed_delta")
        if (N, P) != (self.N, self.P) or d.device != q.device:
            raise ValueError(f"embed_delta: d is {tuple(d.shape)} on {d.device}, q {tuple(q.shape)} on {q.device}")
        if self.N > 1 << 20 or max(self.q_pitch, self.d_pitch) >= 2 ** 31:
            raise ValueError(f"embed_delta: {self.N} frames at pitches {self.q_pitch}, {self.d_pitch} (at most 2^20 frames, pitches below 2^31)")
        self.q, self.d = q, d
        self.stats = torch.zeros(self.N, C.sizeof(L.DeltaStats) // 8, dtype=torch.int64, device=q.device)

    def launch(self):
        L.check(L.load().bnerv_embed_delta(L.stream(), L.ptr(self.q), self.q_pitch, self.N, self.P, L.ptr(self.d), self.d_pitch, L.ptr(self.stats)),
                "bnerv_embed_delta")
        return self

    def check(self):
        return self

    def host(self):
        import numpy as np
        raw = self.stats.cpu().numpy()
        keys = raw[:, 0].copy().view(np.uint32).reshape(-1, 2)             # (max_key, min_key_inv)
        hi = (keys[:, 0] ^ np.uint32(0x80000000)).view(np.int32).astype(np.int64)
        lo = (~keys[:, 1] ^ np.uint32(0x80000000)).view(np.int32).astype(np.int64)
        lo[0] = hi[0] = 0
        return lo, hi, raw[:, 1].copy(), raw[:, 2].copy().view(np.uint64)


class EmbedChainDequant:
    """The symbols of the embedding records of a temporal file resolved and de-quantised, ONE launch (bnerv_embed_chain_dequant):
    q_t = pred[t] ? q_{t-1} + sym_t : sym_t,  out[t] = float(q_t) * scale[t] + beta[t]  (product and sum one fp32 operation each).

        sym        int32 [N, P] device tensor, dense rows at any row pitch and any 4-byte alignment
        pred       N values 0 | 1; pred[0] must be 0 (refused here, before any launch)
        scale, beta  N floats each
        out        fp32 [N, P] device tensor (same rules as sym)
    check() reads the device error word (a host sync) and raises ValueError when a chain left int32."""

    def __init__(self, sym, pred, scale, beta, out):
        import numpy as np
        self.N, self.P, self.sym_pitch = _rows(sym, "sym", torch.int32, "embed_chain_dequant")
        N, P, self.out_pitch = _rows(out, "out", torch.float32, "embed_chain_dequant")
        if (N, P) != (self.N, self.P) or out.device != sym.device:
            raise ValueError(f"embed_chain_dequant: out is {tuple(out.shape)} on {out.device}, sym {tuple(sym.shape)} on {sym.device}")
        pred = np.ascontiguousarray(pred).reshape(-1)
        if pred.size != self.N or ((pred != 0) & (pred != 1)).any():
            raise ValueError(f"embed_chain_dequant: pred must be {self.N} values 0 | 1")
        if pred[0] != 0:
            raise ValueError("embed_chain_dequant: frame 0 is predicted (pred[0] = 1): there is no frame before it")
        coef = np.stack([np.asarray(scale, dtype=np.float32).reshape(-1), np.asarray(beta, dtype=np.float32).reshape(-1)])
        if coef.shape != (2, self.N):
            raise ValueError(f"embed_chain_dequant: scale and beta must have {self.N} entries each")
        if self.N > 65535 * L.CHAIN_SEG or max(self.sym_pitch, self.out_pitch) >= 2 ** 31:
            raise ValueError(f"embed_chain_dequant: {self.N} frames at pitches {self.sym_pitch}, {self.out_pitch}")
        self.sym, self.out = sym, out
        self.pred = _upload(pred.astype(np.uint8), sym.device)
        self.coef = _upload(coef, sym.device).view(torch.float32).reshape(2, self.N)
        self.err = torch.zeros(1, dtype=torch.int32, device=sym.device)

    def launch(self):
        L.check(L.load().bnerv_embed_chain_dequant(L.stream(), L.ptr(self.sym), self.sym_pitch, L.ptr(self.pred), L.ptr(self.coef[0]), L.ptr(self.coef[1]),
                                                   self.N, self.P, L.ptr(self.out), self.out_pitch, L.ptr(self.err)), "bnerv_embed_chain_dequant")
        return self

    def check(self):
        if int(self.err.item()) != 0:
            raise ValueError("embed_chain_dequant: a chain of predicted frames leaves int32 (the file's differences do not belong to its symbols)")
        return self


# ----------------------------------------------------------------------------------------------------------------------
# inter-coded frame embeddings of the post-hoc file (pstream.py, codec.encode_posthoc(..., temporal=True); csrc/hufft.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _byte_rows(t, name, what):
    """(N, P, pitch) of a 2-D uint8 device tensor whose rows are dense (stride 1 along p, any row pitch >= P), at any byte alignment."""
    L.require_device(t, name)
    if t.dim() != 2 or t.dtype != torch.uint8 or t.numel() == 0 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: {name} must be a non-empty [N, P] uint8 device tensor with dense rows (row pitch >= P), got {t.dtype} {tuple(t.shape)} "
                         f"strides {tuple(t.stride())}")
    return int(t.shape[0]), int(t.shape[1]), int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


class EmbedDeltaU8:
    """The frame-to-frame differences of the 8-bit embedding codes and the histograms the choice rule reads, ONE launch (bnerv_embed_delta_u8).

        q          uint8 [N, P] device tensor, dense rows at any row pitch and any byte alignment
        d          None, or the uint8 [N, P] tensor to write (same rules); row 0 is not written
    launch() zeroes the histograms and fills d[t] = (q[t] - q[t - 1]) mod 256 for t >= 1; check() is there for the shape of the other ops (the
    kernel takes no index from a descriptor: nothing can be flagged); host() -> (d, h0, h1): the differences as a uint8 [N, P] numpy array
    (row 0 zero) and the int64 [N, 256] histograms of q[t] and of d[t] (h1[0] is zero)."""

    def __init__(self, q, d=None):
        self.N, self.P, self.q_pitch = _byte_rows(q, "q", "embed_delta_u8")
        self._buf = None
        if d is None:                                      # the histograms and the differences in ONE buffer: host() is one copy
            self._buf = torch.zeros(self.N * (2048 + self.P), dtype=torch.uint8, device=q.device)
            d = self._buf[self.N * 2048:].view(self.N, self.P)
        N, P, self.d_pitch = _byte_rows(d, "d", "embed_delta_u8")
        if (N, P) != (self.N, self.P) or d.device != q.device:
            raise ValueError(f"embed_delta_u8: d is {tuple(d.shape)} on {d.device}, q {tuple(q.shape)} on {q.device}")
        if self.N > 1 << 20 or max(self.q_pitch, self.d_pitch) >= 2 ** 31:
            raise ValueError(f"embed_delta_u8: {self.N} frames at pitches {self.q_pitch}, {self.d_pitch} (at most 2^20 frames, pitches below 2^31)")
        self.q, self.d = q, d
        self.hist = (torch.zeros(self.N * 2048, dtype=torch.uint8, device=q.device) if self._buf is None else self._buf[:self.N * 2048]).view(torch.int32).view(self.N, 2, 256)

    def launch(self):
        L.check(L.load().bnerv_embed_delta_u8(L.stream(), L.ptr(self.q), self.q_pitch, self.N, self.P, L.ptr(self.d), self.d_pitch, L.ptr(self.hist)),
                "bnerv_embed_delta_u8")
        return self

    def check(self):
        return self

    def host(self):
        import numpy as np
        if self._buf is None:
            d, hist = self.d.cpu().numpy().copy(), self.hist.cpu().numpy()
        else:
            raw = self._buf.cpu().numpy()
            d, hist = raw[self.N * 2048:].reshape(self.N, self.P).copy(), raw[:self.N * 2048].view(np.int32).reshape(self.N, 2, 256)
        d[0] = 0
        hist = hist.view(np.uint32).astype(np.int64)
        return d, hist[:, 0].copy(), hist[:, 1].copy()


class HuffDecodeU8(HuffDequant):
    """One bit string of a pstream embedding section on the device: HuffDequant with a byte result (bnerv_huff_decode_u8,
    the same kernel body): out[i] = the symbol, nothing is de-quantised.

        items      one (out, run_bits) per frame: out a contiguous uint8 device tensor (a row of the scratch: any byte alignment)"""
    _name, _entry = "huff_decode_u8", "bnerv_huff_decode_u8"
    _item_struct = L.HuffItemU8
    _item_dtype = [("out", "<u8"), ("n", "<u4"), ("_pad", "<u4")]

    def _item(self, k, item, device):
        out, _ = item
        L.require_device(out, "out")
        n = out.numel()
        if out.dtype != torch.uint8 or not out.is_contiguous() or n == 0 or n >= 2 ** 31 or out.device != device:
            raise ValueError(f"{self._name}: item {k}: out must be a non-empty contiguous uint8 tensor on {device} (below 2^31 elements)")
        return (out.data_ptr(), n, 0)


class EmbedChainDequantU8:
    """The symbols of the embedding section of a pstream file resolved and de-quantised, ONE launch (bnerv_embed_chain_dequant_u8):
    q_t = pred[t] ? (q_{t-1} + sym_t) mod 256 : sym_t,  out = float(min[s]) + float(scale[s]) * float(q)  on the quant_tensor grid of the whole
    [N, P] tensor, s = (i // (red * inner)) * inner + i % inner, i = t * P + p (product and sum one fp32 operation each).

        sym        uint8 [N, P] device tensor, dense rows at any row pitch and any byte alignment
        pred       N values 0 | 1; pred[0] must be 0 (refused here, before any launch)
        lo, step   contiguous fp32 or fp16 device tensors of N * P / red entries each (the grid's min and scale)
        red, inner the grid's geometry; one pair for the whole tensor is (N * P, 1)
        out        fp32 [N, P] device tensor, dense rows at any row pitch, 4-byte aligned
    check() is there for the shape of the other ops: every byte is a code, nothing can be flagged."""

    def __init__(self, sym, pred, lo, step, red, inner, out):
        import numpy as np
        self.N, self.P, self.sym_pitch = _byte_rows(sym, "sym", "embed_chain_dequant_u8")
        N, P, self.out_pitch = _rows(out, "out", torch.float32, "embed_chain_dequant_u8")
        if (N, P) != (self.N, self.P) or out.device != sym.device:
            raise ValueError(f"embed_chain_dequant_u8: out is {tuple(out.shape)} on {out.device}, sym {tuple(sym.shape)} on {sym.device}")
        pred = np.ascontiguousarray(pred).reshape(-1)
        if pred.size != self.N or ((pred != 0) & (pred != 1)).any():
            raise ValueError(f"embed_chain_dequant_u8: pred must be {self.N} values 0 | 1")
        if pred[0] != 0:
            raise ValueError("embed_chain_dequant_u8: frame 0 is predicted (pred[0] = 1): there is no frame before it")
        n, red, inner = self.N * self.P, int(red), int(inner)
        if red < 1 or inner < 1 or n % (red * inner):
            raise ValueError(f"embed_chain_dequant_u8: {n} elements do not split into slices of red={red}, inner={inner}")
        L.require_device(lo, "min"), L.require_device(step, "scale")
        slices = n // red
        if lo.dtype != step.dtype or lo.dtype not in (torch.float32, torch.float16) or lo.numel() != slices or step.numel() != slices \
                or not lo.is_contiguous() or not step.is_contiguous() or (lo.data_ptr() | step.data_ptr()) % lo.element_size():
            raise ValueError(f"embed_chain_dequant_u8: min and scale must be contiguous fp32 or fp16 tensors of {slices} entries each")
        if self.N > 65535 * L.CHAIN_SEG or max(self.sym_pitch, self.out_pitch) >= 2 ** 31 or n >= 2 ** 31:
            raise ValueError(f"embed_chain_dequant_u8: {self.N} frames of {self.P} at pitches {self.sym_pitch}, {self.out_pitch}")
        self.sym, self.out, self.lo, self.step, self.red, self.inner = sym, out, lo, step, red, inner
        self.dtype = L.HUFF_F16 if lo.dtype == torch.float16 else L.HUFF_F32
        self.pred = _upload(pred.astype(np.uint8), sym.device)

    def launch(self):
        L.check(L.load().bnerv_embed_chain_dequant_u8(L.stream(), L.ptr(self.sym), self.sym_pitch, L.ptr(self.pred), L.ptr(self.lo), L.ptr(self.step), self.dtype,
                                                      self.red, self.inner, self.N, self.P, L.ptr(self.out), self.out_pitch), "bnerv_embed_chain_dequant_u8")
        return self

    def check(self):
        return self


def frame_to_u8(x, out=None):
    """[B, 3, H, W] fp32 -> [B, H, W, 3] uint8 = (x.clamp(0, 1) * 255 + 0.5).to(uint8).permute(0, 2, 3, 1) in one pass (the image
    convention of train_nerv_all._save_images).  out: a contiguous uint8 buffer to write into (a captured decode's)."""
    x = L.require_device(x.detach(), "x")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"frame_to_u8: need a non-empty contiguous fp32 [B, 3, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"frame_to_u8: out must be a contiguous uint8 [{B}, {H}, {W}, 3] tensor on {x.device}")
    L.check(L.load().bnerv_frame_to_u8(L.stream(), L.ptr(x), L.ptr(out), B, H, W), "bnerv_frame_to_u8")
    return out


def _raw_bytes(t, name):
    """A contiguous device tensor of raw samples (uint8, or any dtype of file bytes) as its byte count."""
    t = L.require_device(t, name)
    if not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{name}: need a non-empty contiguous device tensor of raw samples")
    return t.numel() * t.element_size()


def yuv420_to_rgb(src, coeffs, B, src_h, src_w, crop=None, frame_stride_bytes=None, out=None):
    """B raw 4:2:0 frames as they lie in a file (src: contiguous device bytes; frame b at byte b * frame_stride_bytes, default: packed) ->
    [B, 3, ch, cw] fp32 RGB in [0, 1] in one launch.  coeffs: yuvio.coefficients(matrix, range, depth);
    crop = (top, left, ch, cw) in source coordinates, any parity (None: the whole frame)."""
    nbytes = _raw_bytes(src, "yuv420_to_rgb: src")
    bps = coeffs.bytes_per_sample
    frame = src_h * src_w * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    top, left, ch, cw = (0, 0, src_h, src_w) if crop is None else (int(v) for v in crop)
    if B < 1 or stride < frame or (B - 1) * stride + frame > nbytes:
        raise ValueError(f"yuv420_to_rgb: {B} frames of {frame} bytes at stride {stride} do not fit the {nbytes} bytes of src")
    if out is None:
        out = torch.empty(B, 3, max(ch, 0), max(cw, 0), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, ch, cw) or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"yuv420_to_rgb: out must be a contiguous fp32 [{B}, 3, {ch}, {cw}] tensor on {src.device}")
    c = coeffs.load_struct()
    L.check(L.load().bnerv_yuv420_to_rgb(L.stream(), L.ptr(src), bps, B, stride, src_h, src_w, top, left, L.ptr(out), ch, cw, C.byref(c)),
            "bnerv_yuv420_to_rgb")
    return out


def rgb_to_yuv420(x, coeffs, out=None, frame_stride_bytes=None):
    """[B, 3, H, W] fp32 (H, W even; values clamped to [0, 1]) -> B raw 4:2:0 frames in file layout, a uint8 [B, frame_stride_bytes] tensor
    (default stride: one frame, 1.5 H W samples of coeffs.bytes_per_sample bytes) in one launch.  coeffs: yuvio.coefficients(...)."""
    x = L.require_device(x.detach(), "x")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"rgb_to_yuv420: need a non-empty contiguous fp32 [B, 3, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    B, _, H, W = x.shape
    bps = coeffs.bytes_per_sample
    frame = H * W * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    if out is None:
        out = torch.empty(B, max(stride, frame), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device or out.numel() < (B - 1) * stride + frame:
        raise ValueError(f"rgb_to_yuv420: out must be a contiguous uint8 tensor of at least {(B - 1) * stride + frame} bytes on {x.device}")
    c = coeffs.store_struct()
    L.check(L.load().bnerv_rgb_to_yuv420(L.stream(), L.ptr(x), B, H, W, L.ptr(out), bps, stride, C.byref(c)), "bnerv_rgb_to_yuv420")
    return out


def _raw_frames(t, name, B, h, w, bps, stride):
    """The frame stride of B raw h x w frames in `t` (contiguous device bytes), checked against its size."""
    nbytes = _raw_bytes(t, name)
    frame = h * w * 3 // 2 * bps
    stride = frame if stride is None else int(stride)
    if B < 1 or stride < frame or (B - 1) * stride + frame > nbytes:
        raise ValueError(f"{name}: {B} frames of {frame} bytes at stride {stride} do not fit its {nbytes} bytes")
    return stride


def yuv420_sse(a, b, B, H, W, bytes_per_sample, src_hw=None, window=(0, 0), a_stride=None, b_stride=None, out=None):
    """The exact sums of squared code differences per frame and plane, [B, 3] int64 (Y, U, V), of B packed H x W frames `a` in file layout
    (what rgb_to_yuv420 writes) against the H x W window at `window` = (top, left), both even, of B raw frames `b` of src_hw = (src_h,
    src_w) (default: H x W) -- one memset and one launch.  a, b: contiguous device bytes, frame k at byte k * stride
    (default: packed).  out: a contiguous int64 [B, 3] device tensor to write into."""
    bps = int(bytes_per_sample)
    if bps not in (1, 2):
        raise ValueError(f"yuv420_sse: bytes_per_sample={bytes_per_sample} (1: yuv420p, 2: yuv420p10le)")
    src_h, src_w = (H, W) if src_hw is None else (int(v) for v in src_hw)
    sa = _raw_frames(a, "yuv420_sse: a", B, H, W, bps, a_stride)
    sb = _raw_frames(b, "yuv420_sse: b", B, src_h, src_w, bps, b_stride)
    if b.device != a.device:
        raise ValueError(f"yuv420_sse: a is on {a.device}, b on {b.device}")
    top, left = (int(v) for v in window)
    if out is None:
        out = torch.empty(B, 3, dtype=torch.int64, device=a.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, 3) or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"yuv420_sse: out must be a contiguous int64 [{B}, 3] tensor on {a.device}")
    L.check(L.load().bnerv_yuv420_sse(L.stream(), L.ptr(a), sa, L.ptr(b), sb, bps, B, H, W, src_h, src_w, top, left, L.ptr(out)), "bnerv_yuv420_sse")
    return out


def yuv_luma_f32(src, bytes_per_sample, B, src_h, src_w, window=None, frame_stride_bytes=None, out=None):
    """The luma window of B raw 4:2:0 frames (src: contiguous device bytes in file layout) as [B, 1, H, W] fp32 = code / maxcode with the
    correctly rounded fp32 division (maxcode 255 at 1 byte per sample, 1023 at 2): the plane MS-SSIM-Y is taken on.
    window = (top, left, H, W) in source coordinates, any parity (None: the whole frame)."""
    bps = int(bytes_per_sample)
    if bps not in (1, 2):
        raise ValueError(f"yuv_luma_f32: bytes_per_sample={bytes_per_sample} (1: yuv420p, 2: yuv420p10le)")
    stride = _raw_frames(src, "yuv_luma_f32: src", B, src_h, src_w, bps, frame_stride_bytes)
    top, left, H, W = (0, 0, src_h, src_w) if window is None else (int(v) for v in window)
    if out is None:
        out = torch.empty(B, 1, max(H, 0), max(W, 0), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 1, H, W) or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"yuv_luma_f32: out must be a contiguous fp32 [{B}, 1, {H}, {W}] tensor on {src.device}")
    L.check(L.load().bnerv_yuv_luma_f32(L.stream(), L.ptr(src), bps, B, stride, src_h, src_w, top, left, L.ptr(out), H, W, 255.0 if bps == 1 else 1023.0),
            "bnerv_yuv_luma_f32")
    return out


YUV_LOSS_STATS = 4         # stats [B, 4] of the plane loss: {L[b], mse_y, mse_u, mse_v}


def _yuv420_loss_launch(pred, src, coeffs, src_hw, window, frame_sel, weights, lam, grad, loss, frame_stride_bytes, accumulate):
    pred = L.require_device(pred, "pred")
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() == 0:
        raise ValueError(f"yuv420_loss: need a non-empty contiguous fp32 [B, 3, H, W] prediction, got {pred.dtype} {tuple(pred.shape)}")
    B, _, H, W = pred.shape
    bps = coeffs.bytes_per_sample
    src_h, src_w = (int(v) for v in src_hw)
    top, left = (int(v) for v in window)
    nbytes = _raw_bytes(src, "yuv420_loss: src")
    if src.device != pred.device:
        raise ValueError(f"yuv420_loss: pred is on {pred.device}, src on {src.device}")
    frame = src_h * src_w * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    if frame <= 0 or stride < frame or nbytes < frame:
        raise ValueError(f"yuv420_loss: frames of {frame} bytes at stride {stride} do not fit the {nbytes} bytes of src")
    n_frames = (nbytes - frame) // stride + 1
    if frame_sel is not None:
        frame_sel = L.require_device(frame_sel, "frame_sel")
        if frame_sel.dtype != torch.float32 or frame_sel.numel() < B or not frame_sel.is_contiguous() or frame_sel.device != pred.device:
            raise ValueError(f"yuv420_loss: frame_sel must hold {B} contiguous fp32 frame numbers on {pred.device}")
    for name, t, shape in (("grad", grad, tuple(pred.shape)), ("loss", loss, None)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != pred.device or
                              (t.numel() != 1 if shape is None else tuple(t.shape) != shape)):
            raise ValueError(f"yuv420_loss: {name} must be a contiguous fp32 {'scalar' if shape is None else list(shape)} tensor on {pred.device}")
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
    stats = torch.empty(B, YUV_LOSS_STATS, dtype=torch.float32, device=pred.device)
    lib = L.load()
    ws_bytes = lib.bnerv_yuv420_loss_ws_bytes(B, H, W)
    ws = _ws(max(ws_bytes, 4), pred.device)
    c = coeffs.store_struct()
    w = (C.c_float * 3)(*(float(v) for v in weights))
    L.check(lib.bnerv_yuv420_loss(L.stream(), L.ptr(pred), B, H, W, L.ptr(src), bps, stride, n_frames, src_h, src_w, top, left, L.ptr(frame_sel),
                                  C.byref(c), w, float(lam), L.ptr(grad), int(accumulate), L.ptr(loss), L.ptr(stats), L.ptr(ws), ws_bytes),
            "bnerv_yuv420_loss")
    return loss, stats, grad


def yuv420_loss_value_grad_stats(pred, src, coeffs, src_hw, window, frame_sel=None, weights=(6, 1, 1), lam=1.0, grad=None, loss=None,
                                 frame_stride_bytes=None, need_grad=True):
    """The plane loss of DESIGN section 33 without an autograd node (the captured step's form): pred [B, 3, H, W] fp32, not clamped, against
    the H x W window at window = (top, left), both even, of raw 4:2:0 frames `src` (contiguous device bytes in file layout, src_hw = (src_h,
    src_w), frame k at byte k * frame_stride_bytes) under coeffs = yuvio.coefficients(...).  Sample b is compared against frame b, or against
    frame int(frame_sel[b]) (fp32 device tensor; clamped to the frames src holds).  Returns (lam * L, stats [B, 4] = {L[b], mse_y, mse_u,
    mse_v}, lam * dL/dpred).  grad and loss handed in: the term is ADDED to them in the same launch (no extra pass over the frame) and they
    are returned; loss handed in alone, or need_grad=False: value and stats only, grad is None."""
    accumulate = loss is not None
    if grad is not None and loss is None:
        raise ValueError("yuv420_loss: a grad to accumulate into needs the loss to accumulate into as well")
    pred = L.f32c(pred.detach())
    if grad is None and need_grad and not accumulate:
        grad = torch.empty_like(pred)
    return _yuv420_loss_launch(pred, src, coeffs, src_hw, window, frame_sel, weights, lam, grad, loss, frame_stride_bytes, accumulate)


class _Yuv420Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, src, coeffs, src_hw, window, frame_sel, weights, frame_stride_bytes):
        p = L.f32c(pred.detach())
        grad = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        loss, stats, grad = _yuv420_loss_launch(p, src, coeffs, src_hw, window, frame_sel, weights, 1.0, grad, None, frame_stride_bytes, False)
        ctx.grad = grad
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, gl, _gs):
        _enter_backward()
        g = ctx.grad
        ctx.grad = None
        return (g * gl if g is not None else None), None, None, None, None, None, None, None


def yuv420_loss(pred, src, coeffs, src_hw, window, frame_sel=None, weights=(6, 1, 1), frame_stride_bytes=None):
    """The plane loss as an autograd function (the eager steps): returns (L [scalar], stats [B, 4]); see yuv420_loss_value_grad_stats."""
    return _Yuv420Loss.apply(pred, src, coeffs, src_hw, window, frame_sel, tuple(float(v) for v in weights), frame_stride_bytes)


# ---- the MS-SSIM-Y term: luma pair -> the loss call at C = 1 -> the gradient back onto the RGB planes ----
MSSSIM_MIN_SIDE = 160      # the five-scale pyramid needs min(H, W) > 160


def luma_grad_consts(coeffs):
    """k_c = d_0 M[0, c] / m in float64: d Yp / d P[c] of the luma plane of DESIGN section 37."""
    return tuple(float(coeffs.denom[0]) * float(coeffs.to_yuv[0, c]) / float(coeffs.maxcode) for c in range(3))


def _luma_pair_args(pred, src, coeffs, src_hw, window, frame_sel, frame_stride_bytes, what):
    pred = L.require_device(pred, "pred")
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() == 0:
        raise ValueError(f"{what}: need a non-empty contiguous fp32 [B, 3, H, W] prediction, got {pred.dtype} {tuple(pred.shape)}")
    B = pred.shape[0]
    bps = coeffs.bytes_per_sample
    src_h, src_w = (int(v) for v in src_hw)
    top, left = (int(v) for v in window)
    nbytes = _raw_bytes(src, f"{what}: src")
    if src.device != pred.device:
        raise ValueError(f"{what}: pred is on {pred.device}, src on {src.device}")
    frame = src_h * src_w * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    if frame <= 0 or stride < frame or nbytes < frame:
        raise ValueError(f"{what}: frames of {frame} bytes at stride {stride} do not fit the {nbytes} bytes of src")
    n_frames = (nbytes - frame) // stride + 1
    if frame_sel is not None:
        frame_sel = L.require_device(frame_sel, "frame_sel")
        if frame_sel.dtype != torch.float32 or frame_sel.numel() < B or not frame_sel.is_contiguous() or frame_sel.device != pred.device:
            raise ValueError(f"{what}: frame_sel must hold {B} contiguous fp32 frame numbers on {pred.device}")
    return pred, bps, stride, n_frames, src_h, src_w, top, left, frame_sel


def yuv_luma_pair(pred, src, coeffs, src_hw, window, frame_sel=None, frame_stride_bytes=None):
    """(yp, ys), both [B, 1, H, W] fp32, in one launch: yp = (o_0 + d_0 (M[0] . pred)) / m, the luma code of the prediction [B, 3, H, W] (fp32, NOT
    clamped) before rounding over the peak; ys = the H x W luma window at window = (top, left), any parity, of raw 4:2:0 frames `src` over the
    peak -- the bits of yuv_luma_f32.  src, src_hw, frame_sel, frame_stride_bytes, coeffs: as yuv420_loss_value_grad_stats."""
    pred, bps, stride, n_frames, src_h, src_w, top, left, frame_sel = _luma_pair_args(L.f32c(pred.detach()), src, coeffs, src_hw, window, frame_sel,
                                                                                         frame_stride_bytes, "yuv_luma_pair")
    B, _, H, W = pred.shape
    yp = torch.empty(B, 1, H, W, dtype=torch.float32, device=pred.device)
    ys = torch.empty_like(yp)
    c = coeffs.store_struct()
    L.check(L.load().bnerv_yuv_luma_pair(L.stream(), L.ptr(pred), B, H, W, L.ptr(src), bps, stride, n_frames, src_h, src_w, top, left, L.ptr(frame_sel),
                                         C.byref(c), L.ptr(yp), L.ptr(ys)), "bnerv_yuv_luma_pair")
    return yp, ys


def luma_grad_rgb(gy, k, lam, loss_term, grad=None, loss=None):
    """The adjoint of yuv_luma_pair's prediction side in one launch: gy [B, 1, H, W] -> grad [B, 3, H, W] = lam k_c gy and loss = lam * loss_term,
    written -- or, with grad / loss handed in, ADDED to what they hold (one fma each).  gy None: the loss word alone.  Returns (loss, grad)."""
    loss_term = L.require_device(loss_term, "loss_term")
    accumulate = loss is not None
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=loss_term.device)
    if gy is not None:
        gy = L.f32c(L.require_device(gy, "gy"))
        B, _, H, W = gy.shape
        if grad is None:
            if accumulate:
                raise ValueError("luma_grad_rgb: a loss to accumulate into needs the grad to accumulate into as well")
            grad = torch.empty(B, 3, H, W, dtype=torch.float32, device=gy.device)
        elif grad.dtype != torch.float32 or tuple(grad.shape) != (B, 3, H, W) or not grad.is_contiguous() or grad.device != gy.device:
            raise ValueError(f"luma_grad_rgb: grad must be a contiguous fp32 [{B}, 3, {H}, {W}] tensor on {gy.device}")
    else:
        B, H, W, grad = 1, 1, 1, None
    if loss.dtype != torch.float32 or loss.numel() != 1 or not loss.is_contiguous() or loss.device != loss_term.device:
        raise ValueError(f"luma_grad_rgb: loss must be a contiguous fp32 scalar tensor on {loss_term.device}")
    kk = (C.c_double * 3)(*(float(v) for v in k))
    L.check(L.load().bnerv_luma_grad_rgb(L.stream(), L.ptr(gy), B, H, W, kk, float(lam), L.ptr(grad), int(accumulate), L.ptr(loss_term), L.ptr(loss)),
            "bnerv_luma_grad_rgb")
    return loss, grad


def _yuv420_msssim_launch(pred, src, coeffs, src_hw, window, frame_sel, lam, grad, loss, frame_stride_bytes, need_grad):
    if min(pred.shape[-2:]) <= MSSSIM_MIN_SIDE:
        raise ValueError(f"yuv420_msssim: the five-scale MS-SSIM needs min(H, W) > {MSSSIM_MIN_SIDE}, got {tuple(pred.shape[-2:])}")
    yp, ys = yuv_luma_pair(pred, src, coeffs, src_hw, window, frame_sel, frame_stride_bytes)
    term, stats, gy = _loss_launch(yp, ys, (0.0, 0.0, 1.0, 0.0, 0.0), need_grad)
    loss, grad = luma_grad_rgb(gy, luma_grad_consts(coeffs), lam, term, grad if need_grad else None, loss)
    return loss, stats[:, 3], grad


def yuv420_msssim_value_grad_stats(pred, src, coeffs, src_hw, window, frame_sel=None, lam=1.0, grad=None, loss=None, frame_stride_bytes=None,
                                   need_grad=True):
    """The MS-SSIM-Y term of DESIGN section 37 without an autograd node (the captured step's form): L_ms = mean_b (1 - S[b]), S[b] the
    five-scale MS-SSIM (data range 1) of the prediction's luma code before rounding over the peak against the source luma window over the peak.
    Operands as yuv420_loss_value_grad_stats.  Returns (lam * L_ms, S [B], lam * dL_ms/dpred); three launch groups: yuv_luma_pair, the loss
    call at C = 1, luma_grad_rgb.  grad and loss handed in: the term is ADDED to them and they are returned; loss handed in alone, or
    need_grad=False: value and S only, grad is None."""
    if grad is not None and loss is None:
        raise ValueError("yuv420_msssim: a grad to accumulate into needs the loss to accumulate into as well")
    need_grad = bool(need_grad) and (grad is not None or loss is None)
    return _yuv420_msssim_launch(L.f32c(pred.detach()), src, coeffs, src_hw, window, frame_sel, lam, grad, loss, frame_stride_bytes, need_grad)


class _Yuv420Msssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, src, coeffs, src_hw, window, frame_sel, frame_stride_bytes):
        loss, S, grad = _yuv420_msssim_launch(L.f32c(pred.detach()), src, coeffs, src_hw, window, frame_sel, 1.0, None, None, frame_stride_bytes,
                                              ctx.needs_input_grad[0])
        ctx.grad = grad
        ctx.mark_non_differentiable(S)
        return loss, S

    @staticmethod
    def backward(ctx, gl, _gs):
        _enter_backward()
        g = ctx.grad
        ctx.grad = None
        return (g * gl if g is not None else None), None, None, None, None, None, None


def yuv420_msssim_loss(pred, src, coeffs, src_hw, window, frame_sel=None, frame_stride_bytes=None):
    """The MS-SSIM-Y term as an autograd function (the eager steps): returns (L_ms [scalar], S [B]); see yuv420_msssim_value_grad_stats."""
    return _Yuv420Msssim.apply(pred, src, coeffs, src_hw, window, frame_sel, frame_stride_bytes)


# ----------------------------------------------------------------------------------------------------------------------
# depthwise conv of the ConvNeXt encoder block (first kernels of row N3)
# ----------------------------------------------------------------------------------------------------------------------
class _DWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = L.f32c(L.require_device(x, "x")); w = L.f32c(w); b = None if b is None else L.f32c(b)
        B, Cc, H, W = x.shape
        K = w.shape[-1]
        assert w.shape == (Cc, 1, K, K), w.shape
        y = torch.empty_like(x)
        L.check(L.load().bnerv_dwconv_fwd(L.stream(), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, Cc, H, W, K, 0), "bnerv_dwconv_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        _enter_backward()
        x, w = ctx.saved_tensors
        g = L.f32c(g)
        B, Cc, H, W = x.shape
        K = w.shape[-1]
        lib = L.load()
        nbytes = lib.bnerv_dwconv_wgrad_ws_bytes(B, Cc, H, W, K)
        ws = _ws(nbytes, x.device)
        dwb = torch.empty(Cc, K * K + 1, dtype=torch.float32, device=x.device)
        L.check(lib.bnerv_dwconv_wgrad(L.stream(), L.ptr(x), L.ptr(g), L.ptr(dwb), L.ptr(ws), nbytes, B, Cc, H, W, K, None), "bnerv_dwconv_wgrad")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.check(lib.bnerv_dwconv_fwd(L.stream(), L.ptr(g), L.ptr(w), None, L.ptr(dx), B, Cc, H, W, K, 1), "bnerv_dwconv_fwd(flip)")
        dw = dwb[:, :K * K].reshape(Cc, 1, K, K)
        db = dwb[:, K * K] if ctx.has_b else None
        return dx, dw, db


def dwconv(x, w, b):
    """F.conv2d(x, w, b, padding=K//2, groups=C) for w [C,1,K,K], K odd <= 7 (ConvNeXt Block.dwconv, model_blocks.py:231)."""
    return _DWConv.apply(x, w, b)


LN_CF_MAX_C = 64


class _LayerNormCF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x = L.f32c(L.require_device(x, "x")); w = L.f32c(w); b = L.f32c(b)
        B, Cc = x.shape[:2]
        HW = x[0, 0].numel()
        y = torch.empty_like(x)
        L.check(L.load().bnerv_lncf_fwd(L.stream(), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, Cc, HW, float(eps)), "bnerv_lncf_fwd")
        ctx.save_for_backward(x, w)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, g):
        _enter_backward()
        x, w = ctx.saved_tensors
        g = L.f32c(g)
        B, Cc = x.shape[:2]
        HW = x[0, 0].numel()
        lib = L.load()
        nbytes = lib.bnerv_lncf_bwd_ws_bytes(B, Cc, HW)
        ws = _ws(nbytes, x.device)
        dx = torch.empty_like(x)
        dwb = torch.empty(2, Cc, dtype=torch.float32, device=x.device)
        L.check(lib.bnerv_lncf_bwd(L.stream(), L.ptr(x), L.ptr(w), L.ptr(g), L.ptr(dx), L.ptr(dwb), L.ptr(ws), nbytes, B, Cc, HW, ctx.eps), "bnerv_lncf_bwd")
        return dx, dwb[0], dwb[1], None


def layernorm_cf(x, w, b, eps):
    """LayerNorm over dim 1 of an NCHW tensor, C <= 64 (model_blocks.py:250-270 `LayerNorm`, data_format channels_first)."""
    return _LayerNormCF.apply(x, w, b, eps)


CNX_MLP_DIMS = (16, 32, 48, 64)


class _CnxMlp(torch.autograd.Function):
    """inp + gamma * pwconv2(gelu(pwconv1(x))) on NCHW tensors (ConvNeXt Block tail, model_blocks.py:245-258): one fused forward
    kernel; backward = one fused kernel (dx and the two pixel-contraction operands) + two k = 1 weight-gradient launches."""

    @staticmethod
    def forward(ctx, x, inp, w1, b1, w2, b2, gamma):
        x = L.f32c(L.require_device(x, "x")); inp = L.f32c(inp)
        w1, b1, w2, b2 = (L.f32c(t) for t in (w1, b1, w2, b2))
        # the kernels stage the two [4C x C] matrices with float4 loads and refuse a misaligned one: hand them an aligned copy
        w1, w2 = (t.clone() if t.data_ptr() % 16 else t for t in (w1, w2))
        gm = None if gamma is None else L.f32c(gamma)
        B, Cc, H, W = x.shape
        train = any(ctx.needs_input_grad)
        out = torch.empty_like(x)
        h1 = torch.empty(B, 4 * Cc, H, W, dtype=torch.float32, device=x.device) if train else None
        L.check(L.load().bnerv_cnx_mlp_fwd(L.stream(), L.ptr(x), L.ptr(inp), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(gm), L.ptr(out),
                                           L.ptr(h1), B, Cc, H * W), "bnerv_cnx_mlp_fwd")
        if train:
            ctx.save_for_backward(x, h1, w1, w2, b2, gm)
        ctx.has_gamma = gamma is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        _enter_backward()
        x, h1, w1, w2, b2, gm = ctx.saved_tensors
        dout = L.f32c(dout)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        gbuf, dhbuf = torch.empty_like(h1), torch.empty_like(h1)
        L.check(L.load().bnerv_cnx_mlp_bwd(L.stream(), L.ptr(h1), L.ptr(dout), L.ptr(w1), L.ptr(w2), L.ptr(gm), L.ptr(dx), L.ptr(gbuf), L.ptr(dhbuf),
                                           B, Cc, H * W), "bnerv_cnx_mlp_bwd")
        dw1 = torch.empty(4 * Cc, Cc, 1, 1, dtype=torch.float32, device=dev); db1 = torch.empty(4 * Cc, dtype=torch.float32, device=dev)
        _wgrad(x, dhbuf, dw1, db1, B=B, Cin=Cc, Cout=4 * Cc, H=H, W=W, k=1, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE)
        S = torch.empty(Cc, 4 * Cc, 1, 1, dtype=torch.float32, device=dev); t = torch.empty(Cc, dtype=torch.float32, device=dev)
        _wgrad(gbuf, dout, S, t, B=B, Cin=4 * Cc, Cout=Cc, H=H, W=W, k=1, in_mode=L.IN_PLAIN, g_mode=L.IN_UNSHUFFLE)
        S = S.reshape(Cc, 4 * Cc)
        if ctx.has_gamma:      # [C x 4C] bookkeeping in one launch: dw2 = gamma S, db2 = gamma t, dgamma = rowsum(w2 * S) + b2 t
            S = S.contiguous()
            dw2, db2, dgamma = torch.empty_like(S), torch.empty_like(t), torch.empty_like(t)
            L.check(L.load().bnerv_cnx_param_grads(L.stream(), L.ptr(S), L.ptr(t), L.ptr(w2), L.ptr(b2), L.ptr(gm), L.ptr(dw2), L.ptr(db2),
                                                   L.ptr(dgamma), Cc), "bnerv_cnx_param_grads")
        else:
            dgamma, dw2, db2 = None, S, t
        return dx, dout, dw1.reshape(4 * Cc, Cc), db1, dw2, db2, dgamma


def cnx_mlp(x, inp, w1, b1, w2, b2, gamma):
    """inp + gamma * (w2 gelu(w1 x + b1) + b2) per pixel; x, inp [B, C, H, W], w1 [4C, C], w2 [C, 4C]; C in CNX_MLP_DIMS.
    A w1 / w2 whose data_ptr() is not 16-byte aligned (a view into a flat parameter buffer) is cloned on EVERY forward -- 4C * C floats
    and one copy launch per call; keep these two parameters in allocations of their own if that matters."""
    return _CnxMlp.apply(x, inp, w1, b1, w2, b2, gamma)


# ----------------------------------------------------------------------------------------------------------------------
# loss / metrics
# ----------------------------------------------------------------------------------------------------------------------
LOSS_COEFFS = {            # (c_l1, c_l2, c_ms, c_fft) per hnerv_utils.py:338-385
    "L1": (1.0, 0.0, 0.0, 0.0),
    "L2": (0.0, 1.0, 0.0, 0.0),
    "L1_freq": (60.0, 0.0, 0.0, 1.0),
    "Fusion7": (0.3, 0.7, 0.0, 0.0),
    "Fusion8": (0.5, 0.5, 0.0, 0.0),
    "Fusion10": (0.7, 0.0, 0.3, 0.0),
    "Fusion11": (0.9, 0.0, 0.1, 0.0),
    "Fusion12": (0.8, 0.0, 0.2, 0.0),
    "Fusion10_freq": (60 * 0.7, 0.0, 60 * 0.3, 1.0),
}
SSIM_LOSS_COEFFS = {       # (c_l1, c_l2, c_ss, c_fft) per hnerv_utils.py:342-361, :387-395: the single-scale SSIM term (bnerv_loss_ssim_fwd_bwd)
    "SSIM": (0.0, 0.0, 1.0, 0.0),
    "Fusion1": (0.0, 0.3, 0.7, 0.0),
    "Fusion2": (0.3, 0.0, 0.7, 0.0),
    "Fusion3": (0.0, 0.5, 0.5, 0.0),
    "Fusion4": (0.5, 0.0, 0.5, 0.0),
    "Fusion5": (0.0, 0.7, 0.3, 0.0),
    "Fusion6": (0.7, 0.0, 0.3, 0.0),
    "Fusion9": (0.9, 0.0, 0.1, 0.0),
    "L1_ssim_freq": (60 * 0.7, 0.0, 60 * 0.3, 1.0),
}
SSIM_MIN_SIDE = 11         # the 11-tap window.  The reference skips the filter along a shorter side; this path declines such frames


def loss_coeffs(loss_type):
    """(c_l1, c_l2, c_ms, c_ss, c_fft) of a loss type; NotImplementedError for a name the HIP path does not build."""
    if loss_type in LOSS_COEFFS:
        c1, c2, cm, cf = LOSS_COEFFS[loss_type]
        return (c1, c2, cm, 0.0, cf)
    if loss_type in SSIM_LOSS_COEFFS:
        c1, c2, cs, cf = SSIM_LOSS_COEFFS[loss_type]
        return (c1, c2, 0.0, cs, cf)
    raise NotImplementedError(f"loss type {loss_type!r} is not on the HIP path; supported: {sorted(LOSS_COEFFS) + sorted(SSIM_LOSS_COEFFS)}")


def _loss_plan(pred, loss_type):
    """Coefficients of `loss_type` for this frame size -- checked BEFORE anything touches the device."""
    coeffs = loss_coeffs(loss_type)
    if coeffs[3] and min(pred.shape[-2:]) < SSIM_MIN_SIDE:
        raise NotImplementedError(f"loss type {loss_type!r}: the SSIM window needs min(H, W) >= {SSIM_MIN_SIDE}, got {tuple(pred.shape[-2:])}")
    return coeffs

_fft_ready = set()


def prepare_loss(H, W, ssim=False):
    """Build the FFT twiddle tables for HxW frames (must happen outside hipGraph capture).  ssim: for the single-scale SSIM path, whose
    FFT kernels take prime factors up to 37."""
    if (H, W, ssim) not in _fft_ready:
        name = "bnerv_loss_ssim_prepare" if ssim else "bnerv_fft_prepare"
        L.check(getattr(L.load(), name)(H, W), name)
        _fft_ready.add((H, W, ssim))


def _loss_launch(pred, target, coeffs, need_grad):
    """One fused call: loss value, per-sample stats and (optionally) d loss / d pred."""
    pred = L.f32c(L.require_device(pred, "pred")); target = L.f32c(target.detach())
    B, Cc, H, W = pred.shape
    c1, c2, cm, cs, cf = coeffs
    lib = L.load()
    if cf:
        prepare_loss(H, W, ssim=bool(cs))
    nbytes = lib.bnerv_loss_ssim_ws_bytes(B, Cc, H, W, int(cf != 0)) if cs else lib.bnerv_loss_ws_bytes(B, Cc, H, W, int(cm != 0), int(cf != 0))
    ws = _ws(nbytes, pred.device)
    grad = torch.empty_like(pred) if need_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    stats = torch.empty(B, L.LOSS_STATS, dtype=torch.float32, device=pred.device)
    d = L.LossDesc(L.ptr(pred), L.ptr(target), L.ptr(grad), L.ptr(loss), L.ptr(stats), L.ptr(ws), nbytes, B, Cc, H, W, c1, c2, cm, cf)
    if cs:      # the single-scale SSIM losses: level 0 only, two launches (five with the spectral term)
        L.check(lib.bnerv_loss_ssim_fwd_bwd(L.stream(), C.byref(d), cs), "bnerv_loss_ssim_fwd_bwd")
    else:
        L.check(lib.bnerv_loss_fwd_bwd(L.stream(), C.byref(d)), "bnerv_loss_fwd_bwd")
    return loss, stats, grad


def _mask_hw(mask, like):
    """The [H, W] inpainting mask as the kernels read it: contiguous fp32 on the device of `like` ([B, C, H, W])."""
    mask = L.f32c(L.require_device(mask.detach(), "mask"))
    if tuple(mask.shape) != tuple(like.shape[-2:]) or like.dim() != 4:
        raise ValueError(f"mask {tuple(mask.shape)} does not match the [H, W] of a frame batch {tuple(like.shape)}")
    return mask


def inpaint_head(img, mask, want_inp=False, out_gt_m=None, out_inp=None):
    """(gt_m, inp) = (img * mask, clamp(img * mask, 0, 1) | None) in ONE pass: both sides' target of the masked loss and the masked frame
    an image-consuming model reads (TransformInput.forward, hnerv_utils.py:59-84).  out_*: buffers to write into (a captured step's)."""
    img = L.f32c(L.require_device(img.detach(), "img"))
    mask = _mask_hw(mask, img)
    B, Cc, H, W = img.shape
    gt_m = torch.empty_like(img) if out_gt_m is None else out_gt_m
    inp = out_inp if out_inp is not None else (torch.empty_like(img) if want_inp else None)
    L.check(L.load().bnerv_inpaint_head(L.stream(), L.ptr(img), L.ptr(mask), L.ptr(inp), L.ptr(gt_m), B, Cc, H * W), "bnerv_inpaint_head")
    return gt_m, inp


def _masked_loss_launch(pred, target, mask, coeffs, need_grad, target_masked=None):
    """_loss_launch(pred * mask, target * mask) with the products, the gradient's mask and the UNMASKED per-sample PSNR (stats[:, 4]) from
    this package's streaming kernels: [head,] pred, the unchanged loss launches, PSNR finalize, [grad]."""
    pred = L.f32c(L.require_device(pred, "pred")); target = L.f32c(L.require_device(target.detach(), "target"))
    mask = _mask_hw(mask, pred)
    B, Cc, H, W = pred.shape
    lib = L.load()
    if target_masked is None:
        target_masked, _ = inpaint_head(target, mask)
    pred_m = torch.empty_like(pred)
    nbytes = lib.bnerv_inpaint_ws_bytes(B, Cc, H * W)
    ws = _ws(nbytes, pred.device)
    L.check(lib.bnerv_inpaint_pred(L.stream(), L.ptr(pred), L.ptr(target), L.ptr(mask), L.ptr(pred_m), L.ptr(ws), nbytes, B, Cc, H * W), "bnerv_inpaint_pred")
    loss, stats, grad = _loss_launch(pred_m, target_masked, coeffs, need_grad)
    # after the loss call: its own column 4 is the PSNR of the masked pair, not the number the reference logs (train_nerv_all.py:350)
    L.check(lib.bnerv_inpaint_psnr(L.stream(), L.ptr(ws), nbytes, stats.data_ptr() + 4 * 4, L.LOSS_STATS, B, Cc, H * W), "bnerv_inpaint_psnr")
    if grad is not None:
        L.check(lib.bnerv_inpaint_grad(L.stream(), L.ptr(grad), L.ptr(mask), B, Cc, H * W), "bnerv_inpaint_grad")
    return loss, stats, grad


def loss_value_grad_stats(pred, target, loss_type="Fusion10_freq", mask=None, target_masked=None):
    """(loss [scalar], stats [B,5], d loss/d pred) without an autograd node: the train step seeds pred.backward(grad) with
    the gradient directly (no ones-fill, no grad * 1 pass over the frame) and reads the per-sample PSNR from stats[:, 4].
    mask ([H, W], inpainting): the loss of (pred * mask, target * mask), bit for bit; grad is already multiplied by the mask and
    stats[:, 4] is the PSNR of pred against the UNMASKED target.  target_masked: target * mask where the caller has it (inpaint_head)."""
    coeffs = _loss_plan(pred, loss_type)
    if mask is None:
        loss, stats, grad = _loss_launch(pred.detach(), target, coeffs, True)
    else:
        loss, stats, grad = _masked_loss_launch(pred.detach(), target, mask, coeffs, True, target_masked)
    return loss.reshape(()), stats, grad


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, coeffs, mask):
        if mask is None:
            loss, stats, grad = _loss_launch(pred, target, coeffs, ctx.needs_input_grad[0])
        else:
            loss, stats, grad = _masked_loss_launch(pred, target, mask, coeffs, ctx.needs_input_grad[0])
        ctx.grad = grad
        ctx.mark_non_differentiable(stats)
        return loss.reshape(()), stats

    @staticmethod
    def backward(ctx, gl, _gs):
        _enter_backward()
        g = ctx.grad
        ctx.grad = None
        return (g * gl if g is not None else None), None, None, None


def loss_with_stats(pred, target, loss_type="Fusion10_freq", mask=None):
    """Returns (batch-mean loss [scalar tensor], stats [B,5] = {loss_b, sum|d|, sum d^2, ms_ssim_b, psnr_b}); column 3 carries ssim_b for
    the single-scale SSIM losses (SSIM_LOSS_COEFFS).  mask ([H, W]): the value and gradient of loss_with_stats(pred * mask, target * mask)
    with psnr_b taken against the unmasked target (loss_value_grad_stats)."""
    return _Loss.apply(pred, target, _loss_plan(pred, loss_type), mask)


def psnr(output, gt):
    """-10*log10(mean_{CHW}(output-gt)^2 + 1e-9) per sample, on the device (no host sync)."""
    output = L.f32c(L.require_device(output.detach(), "output")); gt = L.f32c(gt.detach())
    B, Cc, H, W = output.shape
    lib = L.load()
    nbytes = lib.bnerv_psnr_ws_bytes(B, Cc, H, W)
    ws = _ws(nbytes, output.device)
    out = torch.empty(B, dtype=torch.float32, device=output.device)
    L.check(lib.bnerv_psnr(L.stream(), L.ptr(output), L.ptr(gt), L.ptr(out), L.ptr(ws), nbytes, B, Cc, H, W), "bnerv_psnr")
    return out


def msssim(x, y):
    """ms_ssim(x, y, data_range=1, size_average=False) per sample, on the device."""
    x = L.f32c(L.require_device(x.detach(), "x")); y = L.f32c(y.detach())
    B, Cc, H, W = x.shape
    lib = L.load()
    nbytes = lib.bnerv_loss_ws_bytes(B, Cc, H, W, 1, 0)
    ws = _ws(nbytes, x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(lib.bnerv_msssim(L.stream(), L.ptr(x), L.ptr(y), L.ptr(out), L.ptr(ws), nbytes, B, Cc, H, W), "bnerv_msssim")
    return out


def ssim(x, y):
    """ssim(x, y, data_range=1, size_average=False) per sample, on the device: the bits of stats[:, 3] of the SSIM losses."""
    if min(x.shape[-2:]) < SSIM_MIN_SIDE:
        raise NotImplementedError(f"ssim: the window needs min(H, W) >= {SSIM_MIN_SIDE}, got {tuple(x.shape[-2:])}")
    x = L.f32c(L.require_device(x.detach(), "x")); y = L.f32c(y.detach())
    B, Cc, H, W = x.shape
    lib = L.load()
    nbytes = lib.bnerv_loss_ssim_ws_bytes(B, Cc, H, W, 0)
    ws = _ws(nbytes, x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(lib.bnerv_ssim(L.stream(), L.ptr(x), L.ptr(y), L.ptr(out), L.ptr(ws), nbytes, B, Cc, H, W), "bnerv_ssim")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# interpolation from stored embeddings (csrc/interp.hip; hnerv_utils.interp_plan makes the plan)
# ----------------------------------------------------------------------------------------------------------------------
def embed_expand(src, plan, out=None):
    """out [N, ...] from src [S, ...] (fp32, on the device) under `plan` (hnerv_utils.interp_plan: N rows (ia, ib, w), a host array): a
    stored frame's row is copied, a derived frame's row is blended from two stored rows -- ONE launch (bnerv_embed_expand), the bits of
    hnerv_utils.embed_expand_reference.  The plan is validated here (indices inside src, 0 <= w < 1: ValueError) and goes up as one small
    array.  src and out are used in place: contiguous, at any 4-byte boundary (the 16-byte form runs where it can)."""
    from .hnerv_utils import check_interp_plan
    L.require_device(src, "embed_expand: src")
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() < 1 or src.numel() == 0:
        raise ValueError(f"embed_expand: src must be a non-empty contiguous fp32 tensor [S, ...], got {src.dtype} {tuple(src.shape)}")
    S, P = int(src.shape[0]), int(src[0].numel())
    plan = check_interp_plan(plan, S)
    N = int(plan.size)
    if out is None:
        out = torch.empty((N,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    L.require_device(out, "embed_expand: out")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != src.device or tuple(out.shape) != (N,) + tuple(src.shape[1:]):
        raise ValueError(f"embed_expand: out must be a contiguous fp32 tensor {(N,) + tuple(src.shape[1:])} on {src.device}, got {out.dtype} {tuple(out.shape)}")
    lo, hi = out.data_ptr(), out.data_ptr() + 4 * N * P
    if src.data_ptr() < hi and lo < src.data_ptr() + 4 * S * P:
        raise ValueError("embed_expand: src and out overlap")
    plan_dev = _upload(plan, src.device)
    L.check(L.load().bnerv_embed_expand(L.stream(), L.ptr(src), L.ptr(plan_dev), L.ptr(out), S, N, P), "bnerv_embed_expand")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# frame resize (csrc/resize.hip; boosting_nerv_amd/resize.py holds the definition)
# ----------------------------------------------------------------------------------------------------------------------
_resize_tables = {}      # (n_in, n_out, device) -> (packed table on the device, T, LDS span of the row pass)


def _resize_table(n_in, n_out, device):
    """The device table of one axis (resize.pack_table), uploaded once per (n_in, n_out, device).  Raises ValueError over the tap limit."""
    from . import resize as R
    key = (int(n_in), int(n_out), str(device))
    if key not in _resize_tables:
        first, count, w = R.axis_table(n_in, n_out)
        _resize_tables[key] = (_upload(R.pack_table(first, count, w), device).view(torch.int32), int(w.shape[1]), R.strip_span(first, count))
    return _resize_tables[key]


def _spans_overlap(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def resize_bicubic(x, size, clamp=True, out=None, scratch=None):
    """x [B, C, H, W] fp32 on the device -> [B, C, h, w], size = (h, w): the antialiased bicubic of resize.resize_reference, bit for bit.
    Two launches: rows [B*C, H, W] -> [B*C, H, w] into `scratch` (bnerv_resize_rows), columns -> [B*C, h, w] (bnerv_resize_cols), the clamp
    to [0, 1] in the second.  x, out and scratch (a contiguous fp32 tensor of at least B*C*H*w elements) are used in place at any 4-byte
    boundary; the 16-byte forms run where they can.  An axis over the tap limit is refused (ValueError) before any launch."""
    L.require_device(x, "resize_bicubic: x")
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"resize_bicubic: need a non-empty contiguous fp32 [B, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    B, Cc, H, W = (int(v) for v in x.shape)
    h, w = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError(f"resize_bicubic: size {h}x{w}")
    tab_w, T_w, span = _resize_table(W, w, x.device)          # (both tables before any launch: the tap limit is refused here)
    tab_h, T_h, _ = _resize_table(H, h, x.device)
    planes = B * Cc
    if planes > 65535:
        raise ValueError(f"resize_bicubic: {planes} planes (at most 65535 per call)")
    if out is None:
        out = torch.empty(B, Cc, h, w, dtype=torch.float32, device=x.device)
    elif (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (B, Cc, h, w) or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"resize_bicubic: out must be a contiguous fp32 [{B}, {Cc}, {h}, {w}] tensor on {x.device}")
    if _spans_overlap(x, out):
        raise ValueError("resize_bicubic: x and out overlap")
    need = planes * H * w
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
    elif (not scratch.is_cuda or scratch.dtype != torch.float32 or not scratch.is_contiguous() or scratch.numel() < need or scratch.device != x.device
          or _spans_overlap(scratch, x) or _spans_overlap(scratch, out)):
        raise ValueError(f"resize_bicubic: scratch must be a contiguous fp32 tensor of at least {need} elements on {x.device}, apart from x and out")
    lib = L.load()
    L.check(lib.bnerv_resize_rows(L.stream(), L.ptr(x), L.ptr(scratch), L.ptr(tab_w), planes * H, W, w, T_w, span), "bnerv_resize_rows")
    L.check(lib.bnerv_resize_cols(L.stream(), L.ptr(scratch), L.ptr(out), L.ptr(tab_h), planes, H, h, w, T_h, 1 if clamp else 0), "bnerv_resize_cols")
    return out


def resize_to_yuv420(x, size, coeffs, out=None, frame_stride_bytes=None, scratch=None):
    """x [B, 3, h, w] fp32 on the device -> B raw 4:2:0 frames of size = (H, W), both even, in file layout: a uint8 [B, frame_stride_bytes]
    tensor (default stride: one frame) holding the codes of yuvio.to_yuv_reference(resize.resize_reference(x, (H, W)), coeffs) -- what
    rgb_to_yuv420(resize_bicubic(x, (H, W))) writes, without the full-size fp32 frame.  Two launches: rows [B*3, h, w] ->
    [B*3, h, W] into `scratch` (bnerv_resize_rows; a contiguous fp32 tensor of at least B*3*h*W elements), then the column pass fused with the
    store (bnerv_resize_cols_yuv420).  x and scratch are used in place at any 4-byte boundary.  An axis over the tap limit is refused
    (ValueError) before any launch."""
    L.require_device(x, "resize_to_yuv420: x")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"resize_to_yuv420: need a non-empty contiguous fp32 [B, 3, h, w] tensor, got {x.dtype} {tuple(x.shape)}")
    B, _, h, w = (int(v) for v in x.shape)
    H, W = (int(v) for v in size)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"resize_to_yuv420: 4:2:0 needs even dimensions, size is {H}x{W}")
    tab_w, T_w, span = _resize_table(w, W, x.device)          # (both tables before any launch: the tap limit is refused here)
    tab_h, T_h, _ = _resize_table(h, H, x.device)
    if B * 3 > 65535:
        raise ValueError(f"resize_to_yuv420: {B} frames (at most 21845 per call)")
    bps = coeffs.bytes_per_sample
    frame = H * W * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    if stride < frame or (bps == 2 and stride % 2):
        raise ValueError(f"resize_to_yuv420: frame_stride_bytes={stride} for frames of {frame} bytes of {bps}-byte samples")
    if out is None:
        out = torch.empty(B, stride, dtype=torch.uint8, device=x.device)
    elif (not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device or out.numel() < (B - 1) * stride + frame
          or _spans_overlap(out, x)):
        raise ValueError(f"resize_to_yuv420: out must be a contiguous uint8 tensor of at least {(B - 1) * stride + frame} bytes on {x.device}, apart from x")
    need = B * 3 * h * W
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
    elif (not scratch.is_cuda or scratch.dtype != torch.float32 or not scratch.is_contiguous() or scratch.numel() < need or scratch.device != x.device
          or _spans_overlap(scratch, x) or _spans_overlap(scratch, out)):
        raise ValueError(f"resize_to_yuv420: scratch must be a contiguous fp32 tensor of at least {need} elements on {x.device}, apart from x and out")
    lib, c = L.load(), coeffs.store_struct()
    L.check(lib.bnerv_resize_rows(L.stream(), L.ptr(x), L.ptr(scratch), L.ptr(tab_w), B * 3 * h, w, W, T_w, span), "bnerv_resize_rows")
    L.check(lib.bnerv_resize_cols_yuv420(L.stream(), L.ptr(scratch), L.ptr(tab_h), B, h, H, W, T_h, L.ptr(out), bps, stride, C.byref(c)),
            "bnerv_resize_cols_yuv420")
    return out


# ---- the plane loss through the up-sampler (csrc/upyuvloss.hip) ----
_resize_adjoints = {}    # (n_in, n_out, device) -> (packed adjoint table on the device, Ta, LDS span of the row adjoint)


def _resize_adjoint_table(n_in, n_out, device):
    """The device form of resize.adjoint_table, uploaded once per (n_in, n_out, device).  Raises ValueError over the tap limit."""
    from . import resize as R
    key = (int(n_in), int(n_out), str(device))
    if key not in _resize_adjoints:
        first, count, w = R.adjoint_table(n_in, n_out)
        _resize_adjoints[key] = (_upload(R.pack_table(first, count, w), device).view(torch.int32), int(w.shape[1]), R.strip_span(first, count))
    return _resize_adjoints[key]


def _yuv420_up_loss_launch(pred, size, src, coeffs, src_hw, window, frame_sel, weights, lam, grad, loss, frame_stride_bytes, accumulate, need_grad):
    pred = L.require_device(pred, "pred")
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() == 0:
        raise ValueError(f"yuv420_up_loss: need a non-empty contiguous fp32 [B, 3, h, w] prediction, got {pred.dtype} {tuple(pred.shape)}")
    B, _, h, w = (int(v) for v in pred.shape)
    H, W = (int(v) for v in size)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"yuv420_up_loss: 4:2:0 needs even dimensions, size is {H}x{W}")
    if B * 3 > 65535:
        raise ValueError(f"yuv420_up_loss: {B} samples (at most 21845 per call)")
    bps = coeffs.bytes_per_sample
    src_h, src_w = (int(v) for v in src_hw)
    top, left = (int(v) for v in window)
    if top < 0 or left < 0 or top % 2 or left % 2 or src_h % 2 or src_w % 2:
        raise ValueError(f"yuv420_up_loss: the window offset (top {top}, left {left}) and the {src_w}x{src_h} source must be even and not negative")
    if top + H > src_h or left + W > src_w:
        raise ValueError(f"yuv420_up_loss: the {W}x{H} window at (top {top}, left {left}) leaves the {src_w}x{src_h} frame")
    nbytes = _raw_bytes(src, "yuv420_up_loss: src")
    if src.device != pred.device:
        raise ValueError(f"yuv420_up_loss: pred is on {pred.device}, src on {src.device}")
    frame = src_h * src_w * 3 // 2 * bps
    stride = frame if frame_stride_bytes is None else int(frame_stride_bytes)
    if frame <= 0 or stride < frame or nbytes < frame:
        raise ValueError(f"yuv420_up_loss: frames of {frame} bytes at stride {stride} do not fit the {nbytes} bytes of src")
    n_frames = (nbytes - frame) // stride + 1
    if frame_sel is not None:
        frame_sel = L.require_device(frame_sel, "frame_sel")
        if frame_sel.dtype != torch.float32 or frame_sel.numel() < B or not frame_sel.is_contiguous() or frame_sel.device != pred.device:
            raise ValueError(f"yuv420_up_loss: frame_sel must hold {B} contiguous fp32 frame numbers on {pred.device}")
    elif B > n_frames:
        raise ValueError(f"yuv420_up_loss: {B} samples against {n_frames} frames without frame_sel")
    for name, t, shape in (("grad", grad, tuple(pred.shape)), ("loss", loss, None)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != pred.device or
                              (t.numel() != 1 if shape is None else tuple(t.shape) != shape)):
            raise ValueError(f"yuv420_up_loss: {name} must be a contiguous fp32 {'scalar' if shape is None else list(shape)} tensor on {pred.device}")
    from .yuvio import parse_weights
    weights = parse_weights(weights)
    # the four tables before any launch: either tap limit is refused here
    tab_w, T_w, span_w = _resize_table(w, W, pred.device)
    tab_h, T_h, _ = _resize_table(h, H, pred.device)
    if need_grad:
        adj_h, Ta_h, _ = _resize_adjoint_table(h, H, pred.device)
        adj_w, Ta_w, span_a = _resize_adjoint_table(w, W, pred.device)
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
    stats = torch.empty(B, YUV_LOSS_STATS, dtype=torch.float32, device=pred.device)
    lib = L.load()
    ws_bytes = lib.bnerv_yuv420_up_loss_ws_bytes(B, h, w, H, W)
    if ws_bytes == 0:
        raise ValueError(f"yuv420_up_loss: no workspace for B={B}, {w}x{h} -> {W}x{H}")
    ws = _ws(ws_bytes, pred.device)
    c = coeffs.store_struct()
    wv = (C.c_float * 3)(*weights)
    L.check(lib.bnerv_yuv420_up_loss_fwd(L.stream(), L.ptr(pred), B, h, w, H, W, L.ptr(tab_w), T_w, span_w, L.ptr(tab_h), T_h, L.ptr(src), bps, stride,
                                         n_frames, src_h, src_w, top, left, L.ptr(frame_sel), C.byref(c), wv, float(lam), 1 if need_grad else 0,
                                         int(accumulate), L.ptr(loss), L.ptr(stats), L.ptr(ws), ws_bytes), "bnerv_yuv420_up_loss_fwd")
    if need_grad:
        L.check(lib.bnerv_yuv420_up_loss_bwd(L.stream(), B, h, w, H, W, L.ptr(adj_h), Ta_h, L.ptr(adj_w), Ta_w, span_a, C.byref(c), float(lam), L.ptr(grad),
                                             int(accumulate), L.ptr(ws), ws_bytes), "bnerv_yuv420_up_loss_bwd")
    return loss, stats, grad


def yuv420_up_loss_value_grad_stats(pred, size, src, coeffs, src_hw, window, frame_sel=None, weights=(6, 1, 1), lam=1.0, grad=None, loss=None,
                                    frame_stride_bytes=None, need_grad=True):
    """The plane loss at the master's size for a prediction below (or above, or at) it, without an autograd node: pred
    [B, 3, h, w] fp32, not clamped, is up-sampled to size = (H, W), both even, by the table filter of resize.py without its clamp, and that
    frame -- never stored -- is compared against the H x W window at window = (top, left), both even, of raw 4:2:0 frames `src`; everything
    else (src, coeffs, src_hw, frame_sel, weights, lam, frame_stride_bytes, stats) as yuv420_loss_value_grad_stats.  Returns (lam * L, stats
    [B, 4] = {L[b], mse_y, mse_u, mse_v} at the master's size, lam * dL/dpred [B, 3, h, w], the exact adjoint).  grad and loss handed in: the
    term is ADDED to them and they are returned; loss handed in alone, or need_grad=False: value and stats only, grad is None.  Five launches
    (three value-only); an odd size, a window that leaves the source, a table over its tap limit and a wrong grad / loss are refused
    (ValueError) before any launch."""
    accumulate = loss is not None
    if grad is not None and loss is None:
        raise ValueError("yuv420_up_loss: a grad to accumulate into needs the loss to accumulate into as well")
    pred = L.f32c(pred.detach())
    if grad is None and need_grad and not accumulate:
        grad = torch.empty_like(pred)
    return _yuv420_up_loss_launch(pred, size, src, coeffs, src_hw, window, frame_sel, weights, lam, grad, loss, frame_stride_bytes, accumulate,
                                  grad is not None)


class _Yuv420UpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, size, src, coeffs, src_hw, window, frame_sel, weights, frame_stride_bytes):
        p = L.f32c(pred.detach())
        grad = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        loss, stats, grad = _yuv420_up_loss_launch(p, size, src, coeffs, src_hw, window, frame_sel, weights, 1.0, grad, None, frame_stride_bytes, False,
                                                   grad is not None)
        ctx.grad = grad
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, gl, _gs):
        _enter_backward()
        g = ctx.grad
        ctx.grad = None
        return (g * gl if g is not None else None), None, None, None, None, None, None, None, None


def yuv420_up_loss(pred, size, src, coeffs, src_hw, window, frame_sel=None, weights=(6, 1, 1), frame_stride_bytes=None):
    """The plane loss through the up-sampler as an autograd function (the eager steps): returns (L [scalar], stats [B, 4]); see
    yuv420_up_loss_value_grad_stats."""
    return _Yuv420UpLoss.apply(pred, tuple(int(v) for v in size), src, coeffs, src_hw, window, frame_sel, tuple(float(v) for v in weights),
                               frame_stride_bytes)


# ----------------------------------------------------------------------------------------------------------------------
# global magnitude pruning (csrc/prune.hip; boosting_nerv_amd/prune.py drives it)
# ----------------------------------------------------------------------------------------------------------------------
class PruneTable:
    """The device descriptor table of bnerv_kth_abs / bnerv_prune_masks / bnerv_mask_mul over fp32 tensors (and their uint8 masks): one
    (tensor, mask, n) item per tensor and one (item, first element) pair per slice of PRUNE_SLICE elements, uploaded once.  The tensors are
    used IN PLACE: contiguous fp32 device tensors at any 4-byte boundary, masks contiguous uint8 of the same element count at any byte.
    `key` names every address the table holds: whoever caches a table compares it."""

    def __init__(self, tensors, masks=None, what="prune table"):
        import numpy as np
        tensors = list(tensors)
        if not tensors:
            raise ValueError(f"{what}: no tensors")
        if masks is not None and len(masks) != len(tensors):
            raise ValueError(f"{what}: {len(tensors)} tensors and {len(masks)} masks")
        for t in tensors + list(masks or []):
            L.require_device(t, what)
        device = tensors[0].device
        table = np.zeros(len(tensors), dtype=np.dtype([("x", "<u8"), ("mask", "<u8"), ("n", "<u4"), ("_pad", "<u4")]))
        assert table.dtype.itemsize == C.sizeof(L.PruneItem)
        blocks, total = [], 0
        for k, t in enumerate(tensors):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0 or t.numel() >= 2 ** 31 or t.device != device:
                raise ValueError(f"{what}: tensor {k} must be a non-empty contiguous fp32 tensor on {device} (below 2^31 elements)")
            m = None if masks is None else masks[k]
            if m is not None and (m.dtype != torch.uint8 or not m.is_contiguous() or m.numel() != t.numel() or m.device != device):
                raise ValueError(f"{what}: mask {k} must be a contiguous uint8 tensor of {t.numel()} elements on {device}")
            table[k] = (t.data_ptr(), 0 if m is None else m.data_ptr(), t.numel(), 0)
            first = np.arange(0, t.numel(), L.PRUNE_SLICE, dtype=np.uint32)
            blocks.append(np.stack([np.full(first.size, k, dtype=np.uint32), first], axis=1))
            total += t.numel()
        if total >= 2 ** 32:
            raise ValueError(f"{what}: {total} elements (a table holds fewer than 2^32)")
        blocks = np.concatenate(blocks)
        self.key = tuple((int(r["x"]), int(r["mask"]), int(r["n"])) for r in table)
        self.items, self.blocks = _upload(table, device), _upload(blocks, device)
        self.n_items, self.n_blocks, self.total, self.device = len(tensors), int(blocks.shape[0]), total, device
        self.has_masks = masks is not None
        self._keep = (tensors, masks)

    def _args(self):
        return L.ptr(self.items), self.n_items, L.ptr(self.blocks), self.n_blocks

    def kth_abs(self, k, out=None):
        """Launches the select; -> out, int32 [4] on the device: (bits of tau, flags, pruned count low, high).  See kth_abs()."""
        k = int(k)
        if not 1 <= k <= self.total:
            raise ValueError(f"kth_abs: k = {k} outside 1..{self.total}")
        if out is None:
            out = torch.zeros(4, dtype=torch.int32, device=self.device)
        L.check(L.load().bnerv_kth_abs(L.ctx().handle, L.stream(), *self._args(), k, L.ptr(out)), "bnerv_kth_abs")
        return out

    def prune_masks(self, tau):
        if not self.has_masks:
            raise ValueError("prune_masks: the table was built without masks")
        if tau.dtype not in (torch.float32, torch.int32) or tau.numel() < 1 or tau.device != self.device:
            raise ValueError(f"prune_masks: tau must be a float32 (or int32 bit pattern) tensor on {self.device}")
        L.check(L.load().bnerv_prune_masks(L.stream(), *self._args(), L.ptr(tau)), "bnerv_prune_masks")

    def mask_mul(self):
        if not self.has_masks:
            raise ValueError("mask_mul: the table was built without masks")
        L.check(L.load().bnerv_mask_mul(L.stream(), *self._args()), "bnerv_mask_mul")


KTH_FLAG_NAN, KTH_FLAG_RANK, KTH_FLAG_DESC = 1, 2, 4      # flag word of bnerv_kth_abs


def kth_abs(tensors, k, return_flags=False):
    """(tau, n_pruned) as device tensors, no host sync: tau (float32 [1]) is the k-th smallest |w| over ALL tensors (1-based, exact: a radix
    select on the bit patterns, the same bits on every device and in every run) and n_pruned (int64 [1]) counts the elements with
    |w| <= tau.  return_flags: a third int32 [1] tensor, KTH_FLAG_NAN set when a tensor holds a NaN."""
    tensors = list(tensors)
    for t in tensors:
        L.require_device(t, "kth_abs: tensor")
    out = PruneTable(tensors, None, "kth_abs").kth_abs(k)
    res = (out[0:1].view(torch.float32), out[2:4].view(torch.int64))
    return res + (out[1:2],) if return_flags else res


def prune_masks(tensors, masks, tau):
    """masks[j][i] = |tensors[j][i]| > tau (uint8 1 / 0), tensors[j] *= masks[j]: one launch, in place; tau a device tensor (kth_abs)."""
    for t in list(tensors) + list(masks):
        L.require_device(t, "prune_masks: tensor")
    PruneTable(tensors, list(masks), "prune_masks").prune_masks(tau)


def mask_mul(tensors, masks):
    """tensors[j] *= masks[j] (fp32 by uint8) for the whole list in ONE launch, in place."""
    for t in list(tensors) + list(masks):
        L.require_device(t, "mask_mul: tensor")
    PruneTable(tensors, list(masks), "mask_mul").mask_mul()
