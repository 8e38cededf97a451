"""The train step of train_nerv_all.py:328-350 as one object: (inpainting mask ->) forward -> loss -> backward -> (gradient all-reduce)
-> (pruning: gradient mask) -> (global-norm clip) -> Adan / Adam, with per-step PSNR accumulated on the device.  After a few eager steps the fixed-shape step is captured into hipGraphs and
replayed (≈100 short kernels per step: launch latency, not arithmetic, is what a Python-driven loop would pay for).

  world == 1 :  one graph   [fwd, loss, bwd, (clip,) Adan]
  world  > 1 :  one graph   [fwd, loss, bwd, bucket-gather, RCCL all-reduce of ONE flat bucket, bucket-scatter, (clip,) Adan]
                (two graphs around an eager all-reduce when the collective cannot be captured: gloo in the CPU-transport tests)

Everything that changes per step and is not data (lr, Adan bias corrections) lives in device memory written by
Adan.prepare_step(), so the captured kernels never see a stale scalar."""
import torch

from . import hnerv_utils as hu  # noqa: F401
from . import ops
from .dp import GradBucket


class YuvTerm:
    """What a step needs to add the plane loss of DESIGN section 33 (ops.yuv420_loss) to its loss: `raw`, the resident raw 4:2:0 clip in
    file layout (YuvFile.raw_to_device: a uint8 device tensor, frame k at byte k * frame_stride_bytes); coeffs = yuvio.coefficients(...);
    src_hw = (src_h, src_w) of a raw frame; window = (top, left) of the training crop in it, both even; the plane weights; lam, the factor
    of the term in the total loss; pure: the term is the whole loss (--loss YUV420), the RGB loss is not launched.  lam_ms > 0 adds lam_ms
    times the MS-SSIM-Y term of DESIGN section 37 (ops.yuv420_msssim_loss) against the same window's luma; lam may then be 0 (no plane MSE).
    up = (H, W): the prediction is smaller (or larger) than the window; the loss is taken at the window's H x W through the up-sampler
    (ops.yuv420_up_loss), which has no MS-SSIM-Y form."""

    def __init__(self, raw, coeffs, src_hw, window, weights=(6, 1, 1), lam=1.0, pure=False, frame_stride_bytes=None, lam_ms=0.0, up=None):
        from . import yuvio
        self.raw, self.coeffs = raw, coeffs
        self.src_hw = tuple(int(v) for v in src_hw)
        self.window = tuple(int(v) for v in window)
        self.weights = yuvio.parse_weights(weights)
        self.lam, self.pure, self.frame_stride_bytes = float(lam), bool(pure), frame_stride_bytes
        if self.window[0] % 2 or self.window[1] % 2 or min(self.window) < 0:
            raise ValueError(f"YuvTerm: the crop offset (top {self.window[0]}, left {self.window[1]}) must be even: a 4:2:0 chroma sample covers a 2x2 block of the source")
        self.lam_ms = float(lam_ms)
        if not self.lam_ms >= 0 or self.lam_ms == float("inf"):
            raise ValueError(f"YuvTerm: lam_ms={lam_ms} (a finite factor >= 0; 0 switches the MS-SSIM-Y term off)")
        if not (self.lam > 0 or (self.lam_ms > 0 and self.lam == 0)):
            raise ValueError(f"YuvTerm: lam={lam} (a positive factor; leave the term out to switch it off)")
        self.ms_out = None                                   # S [B] of the last autograd_term() call with lam_ms > 0
        self.up = None if up is None else tuple(int(v) for v in up)
        if self.up is not None:
            if len(self.up) != 2 or min(self.up) < 2 or self.up[0] % 2 or self.up[1] % 2:
                raise ValueError(f"YuvTerm: up={up} (the window's size (H, W), both even)")
            if self.lam_ms > 0:
                raise ValueError("YuvTerm: the MS-SSIM-Y term has no form through the up-sampler: up with lam_ms > 0")

    def check_frame(self, H, W):
        if self.up is not None:                              # the window is the master's, whatever size the prediction has
            if H < 1 or W < 1:
                raise ValueError(f"YuvTerm: the frames are {H}x{W}")
            H, W = self.up
        if H % 2 or W % 2:
            raise ValueError(f"YuvTerm: 4:2:0 needs an even crop, the frames are {H}x{W}")
        if self.window[0] + H > self.src_hw[0] or self.window[1] + W > self.src_hw[1]:
            raise ValueError(f"YuvTerm: the {H}x{W} crop at {self.window} leaves the {self.src_hw[0]}x{self.src_hw[1]} source frame")
        if self.lam_ms > 0 and min(H, W) <= ops.MSSSIM_MIN_SIDE:
            raise ValueError(f"YuvTerm: the five-scale MS-SSIM-Y term needs min(H, W) > {ops.MSSSIM_MIN_SIDE}, the frames are {H}x{W}")

    def kwargs(self):
        return dict(weights=self.weights, frame_stride_bytes=self.frame_stride_bytes)

    def value_grad_stats(self, out, sel, **kw):
        """ops.yuv420_loss_value_grad_stats of this term, or its form through the up-sampler with `up` set."""
        if self.up is None:
            return ops.yuv420_loss_value_grad_stats(out, self.raw, self.coeffs, self.src_hw, self.window, sel, **kw, **self.kwargs())
        return ops.yuv420_up_loss_value_grad_stats(out, self.up, self.raw, self.coeffs, self.src_hw, self.window, sel, **kw, **self.kwargs())

    def loss(self, out, sel):
        """(L with its autograd node, stats [B, 4]): ops.yuv420_loss, or ops.yuv420_up_loss with `up` set."""
        if self.up is None:
            return ops.yuv420_loss(out, self.raw, self.coeffs, self.src_hw, self.window, sel, **self.kwargs())
        return ops.yuv420_up_loss(out, self.up, self.raw, self.coeffs, self.src_hw, self.window, sel, **self.kwargs())

    def autograd_term(self, out, sel):
        """(lam * L + lam_ms * L_ms with its autograd nodes, plane stats [B, 4] | None, S [B] | None) for the eager steps: sample b of `out`
        against raw frame int(sel[b]) (fp32 device tensor).  A factor at 0 launches nothing for its part."""
        total = stats = ms = None
        if self.lam > 0:
            term, stats = self.loss(out, sel)
            total = self.lam * term
        if self.lam_ms > 0:
            term, ms = ops.yuv420_msssim_loss(out, self.raw, self.coeffs, self.src_hw, self.window, sel, frame_stride_bytes=self.frame_stride_bytes)
            total = self.lam_ms * term if total is None else total + self.lam_ms * term
        self.ms_out = ms
        return total, stats, ms


class TrainStep:
    def __init__(self, model, optimizer, loss_type, takes_image, batch_shape, device, use_graph=True, warmup_eager=3,
                 process_group=None, world_size=1, clip_max_norm=0.0, force_bucket=False, dp_buckets=None, mask=None, prune=None, yuv=None):
        self.model, self.opt, self.loss_type = model, optimizer, loss_type
        # prune (prune.Pruner of this model and optimizer): the gradients of the prunable tensors are multiplied by their masks in one
        # launch after the exchange, in front of the clip and the update (_clip_grads).  The masks keep their addresses, so an event
        # between two replays (Pruner.prune_to) changes weights, masks and optimizer state in place and needs no re-capture.
        if prune is not None:
            if type(self) is not TrainStep:
                raise NotImplementedError(f"{type(self).__name__}: pruning is built for the plain train step only")
            if prune.optimizer is not optimizer or not hasattr(optimizer, "launch_grad_mask"):
                raise ValueError("TrainStep: prune must be a prune.Pruner of this model and of this step's fused optimizer")
        self.prune = prune
        self.takes_image = takes_image                       # HNeRV_Boost consumes the frame; NeRV/ENeRV the frame index
        self.dev = device
        B, C, H, W = batch_shape
        self.static_img = torch.zeros(B, C, H, W, dtype=torch.float32, device=device)
        self.static_idx = torch.zeros(B, dtype=torch.float64, device=device)
        self.use_graph = use_graph
        self.clip_max_norm = clip_max_norm                   # > 0: optimizer.launch_clip() on the (averaged) gradients, in front of the update
        # mask [H, W] (--inpanting, hnerv_utils.TransformInput): the loss sees (out * mask, frame * mask), an image-consuming model reads
        # clamp(frame * mask, 0, 1), and psnr_out stays the PSNR against the unmasked frame (train_nerv_all.py:331-350 of the reference)
        self.mask = self.static_gtm = self.static_in = None
        if mask is not None:
            if tuple(mask.shape) != (H, W):
                raise ValueError(f"TrainStep: mask {tuple(mask.shape)} for frames of {(H, W)}")
            self.mask = mask.detach().to(device=device, dtype=torch.float32).contiguous()
            self.static_gtm = torch.zeros_like(self.static_img)
            self.static_in = torch.zeros_like(self.static_img) if takes_image else None
        # yuv (YuvTerm): the plane loss against the raw source is added to the loss -- value and gradient -- by one more launch behind the
        # RGB loss (or replaces it: yuv.pure).  The frame number(s) it compares against are device words: the schedule record's on a bound
        # clip, yuv_sel (refreshed by a device copy in __call__) otherwise.  yuv_stats_out: its [B, 4] stats {L[b], mse_y, mse_u, mse_v}
        # (None with yuv.lam == 0).  yuv.lam_ms > 0: the MS-SSIM-Y term's three launch groups go behind it and add into the same loss and
        # gradient; yuv_ms_out: its S [B]
        self.yuv, self.yuv_sel, self.yuv_stats_out, self.yuv_ms_out = yuv, None, None, None
        if yuv is not None:
            if mask is not None:
                raise ValueError("TrainStep: the plane loss has no masked (inpainting) form: give a mask or yuv, not both")
            yuv.check_frame(H, W)
            self.yuv_sel = torch.zeros(B, dtype=torch.float32, device=device)
        self.warmup_eager = warmup_eager
        self.n_calls = 0
        self.graph_a = self.graph_b = None
        self.collective_in_graph = False
        self._opt_epoch = getattr(optimizer, "state_epoch", 0)
        self.loss_out = self.psnr_out = None
        self.world = world_size
        # force_bucket: run the multi-GPU code path (bucket gather -> RCCL all-reduce -> scatter, two graphs) on a 1-rank
        # group, so the path the scaling runs take can be tested on a single-GPU box
        # dp_buckets == 2 (or BNERV_DP_BUCKETS=2): the bucket in two segments -- the decoder layers' gradients start their all-reduce on a
        # side stream from an autograd hook at the decoder / stem boundary, next to the rest of the backward (dp.GradBucket); needs a
        # model that names its late parameters and calls the hook (model_nerv.NeRV_Boost).  Default 1: see DESIGN section 5.
        # Two segments are valid only where every early (decoder) gradient is COMPLETE when the stem-output hook fires: the plain
        # step.  A subclass whose backward finishes parameter gradients later (CompressionStep: the convs consume de-quantised weights,
        # the real weight / quantiser gradients appear in the CEM backward, after the hook) would gather zeros for them -- so the
        # environment switch is honoured by TrainStep itself only, and exchange_early() refuses a segment with a missing gradient.
        import os as _os
        if dp_buckets is None:
            dp_buckets = int(_os.environ.get("BNERV_DP_BUCKETS", "1")) if type(self) is TrainStep else 1
        nb = int(dp_buckets)
        if nb == 2 and type(self) is not TrainStep:
            raise ValueError(f"{type(self).__name__}: dp_buckets=2 needs a backward whose decoder gradients are final at the stem boundary "
                             "(the plain TrainStep); use one bucket")
        late = model.dp_late_parameters() if (nb == 2 and hasattr(model, "dp_late_parameters")) else None
        self.bucket = GradBucket(model.parameters(), process_group, force=force_bucket, late_params=late) if (world_size > 1 or force_bucket) else None
        self._early_ok = True                                # False while a graph that cannot hold the collective is being captured
        if self.bucket is not None and self.bucket.two:
            model.dp_hook = self._dp_hook
        self.params = [p for p in model.parameters() if p.requires_grad]
        self._fetching = False                               # inside step_frame(): the step starts with the frame fetch
        self._wplan_entries = 0                              # entries of the capture stream context's weight-fragment plan
        self._clip = self._clip_norms = None                 # bind_clip(): the resident clip step_frame() picks its frame from

    # ---- pieces -------------------------------------------------------------------------------------------------------
    def bind_clip(self, frames, norms):
        """The clip this step trains on, resident on the device: frames [N, C, H, W] fp32, norms [N] fp64 ((idx + 1) / N,
        hnerv_utils.py:47).  step_frame(i) then trains frame i with ONE host -> device copy per step (the 32-byte schedule record that
        also carries i) instead of two device copies and that record: the frame is fetched by the first launch of the (captured) step.
        Needs the Adan optimizer of this package (its schedule record carries the index)."""
        if not hasattr(self.opt, "finish_capture"):
            raise TypeError("bind_clip needs the fused Adan optimizer (its device schedule record carries the frame index)")
        assert frames.shape[1:] == self.static_img.shape[1:] and self.static_img.shape[0] == 1, "bind_clip: one frame per step"
        self._clip = frames.contiguous()
        self._clip_norms = norms.to(torch.float64).contiguous()
        self.graph_a = self.graph_b = None

    def _fetch(self):
        from . import _lib as L
        sel = self.opt._sched[0][1]
        L.check(L.load().bnerv_fetch_frame(L.stream(), L.ptr(self._clip), L.ptr(self._clip_norms), sel.data_ptr() + 5 * 4, self._clip.shape[0],
                                           self._clip[0].numel(), L.ptr(self.static_img), L.ptr(self.static_idx)), "bnerv_fetch_frame")

    def _fwd_bwd(self):
        if self._fetching and not getattr(self, "_fetch_done", False):
            self._fetch()
        self.opt.zero_grad(set_to_none=True)
        if self.mask is not None:
            ops.inpaint_head(self.static_img, self.mask, out_gt_m=self.static_gtm, out_inp=self.static_in)
        inp = (self.static_img if self.mask is None else self.static_in) if self.takes_image else self.static_idx
        img_out, _, _ = self.model(inp, norm_idx=self.static_idx)
        # loss_fn(...).backward() + psnr_fn_single(...) of train_nerv_all.py:337-347 as ONE fused launch sequence: the loss
        # gradient seeds backward directly and the per-sample PSNR comes from the same L2 sums (stats[:, 4]).  With a mask the gradient
        # comes back masked and stats[:, 4] is the PSNR against the unmasked frame (ops.loss_value_grad_stats)
        if self.yuv is None:
            loss, stats, grad = ops.loss_value_grad_stats(img_out, self.static_img, self.loss_type, mask=self.mask, target_masked=self.static_gtm)
            psnr = stats[:, 4]
        else:
            loss, psnr, grad = self._yuv_loss(img_out)
        if self._lazy_flush_valid():
            # (dx_ok: the model's first block hands its queued input gradient to an operator of this package, which flushes on entry -- ops._end_block)
            with ops.lazy_flush(dx_ok=getattr(self.model, "lazy_dx_ok", False)):      # slab reductions are flushed by their first reader, not per block
                img_out.backward(grad)
        else:
            img_out.backward(grad)
        self.loss_out = loss
        self.psnr_out = psnr

    def _yuv_sel(self):
        """The device word(s) the plane loss reads its frame number(s) from: on a bound clip the one the frame fetch reads."""
        return self.opt._sched[0][1][5:6] if self._fetching else self.yuv_sel

    def _yuv_loss(self, img_out):
        """(loss, psnr [B], grad) with the plane loss: added by its own launch into the RGB loss call's loss and gradient (no further pass
        over the frame), or alone (yuv.pure; the PSNR then comes from ops.psnr)."""
        y = self.yuv
        if y.lam_ms > 0:
            return self._yuv_ms_loss(img_out)
        if y.pure:
            loss, self.yuv_stats_out, grad = y.value_grad_stats(img_out, self._yuv_sel(), lam=y.lam)
            return loss, ops.psnr(img_out.detach(), self.static_img), grad
        loss, stats, grad = ops.loss_value_grad_stats(img_out, self.static_img, self.loss_type)
        _, self.yuv_stats_out, _ = y.value_grad_stats(img_out, self._yuv_sel(), lam=y.lam, grad=grad, loss=loss)
        return loss, stats[:, 4], grad

    def _yuv_ms_loss(self, img_out):
        """_yuv_loss with the MS-SSIM-Y term (yuv.lam_ms > 0): the launches in front of it are those of lam_ms == 0 -- the RGB loss unless pure,
        the plane MSE unless lam == 0 -- and the term adds into their loss and gradient (or, pure with lam == 0, writes them)."""
        y = self.yuv
        loss = grad = psnr = None
        if not y.pure:
            loss, stats, grad = ops.loss_value_grad_stats(img_out, self.static_img, self.loss_type)
            psnr = stats[:, 4]
        if y.lam > 0:
            loss, self.yuv_stats_out, grad = y.value_grad_stats(img_out, self._yuv_sel(), lam=y.lam, grad=grad, loss=loss)
        loss, self.yuv_ms_out, grad = ops.yuv420_msssim_value_grad_stats(img_out, y.raw, y.coeffs, y.src_hw, y.window, self._yuv_sel(), lam=y.lam_ms,
                                                                         grad=grad, loss=loss, frame_stride_bytes=y.frame_stride_bytes)
        return loss, (ops.psnr(img_out.detach(), self.static_img) if psnr is None else psnr), grad

    def _lazy_flush_valid(self):
        """Lazy flushing (ops.lazy_flush) lets backward RETURN weight / bias gradients and TAT channel sums whose slab reductions are
        still queued; only this package's operators (grouped dense, dense GEMM, stand-alone affine) flush before reading.  The invariant
        that makes this safe -- checked here, every step, not only promised by the model's `lazy_flush_ok` flag -- is that NOTHING else
        reads a gradient inside the backward: no parameter holds a .grad (AccumulateGrad would add into it: zero_grad(set_to_none=True)
        above), no parameter carries a tensor hook, and no module carries backward hooks.  Anything else takes the per-block flush."""
        import os
        if os.environ.get("BNERV_LAZY_FLUSH", "1") == "0" or not getattr(self.model, "lazy_flush_ok", False):
            return False
        for p in self.params:
            if p.grad is not None or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
                return False
        for m in self.model.modules():
            if m._backward_hooks or m._backward_pre_hooks:
                return False
        return True

    def _planned_fwd_bwd(self):
        """_fwd_bwd inside a capture: the weight fragments of every wide split conv call of the step come from ONE launch at the
        start (the context's frozen plan, include/bnerv.h bnerv_ctx_wplan_*) -- the weights only change in the Adan launch after
        backward.  Without a plan this is _fwd_bwd."""
        from . import _lib as L
        if not self._wplan_entries:
            return self._fwd_bwd()
        lib, c = L.load(), L.ctx()
        fetched = False
        if self._fetching:
            # the plan's launch carries the frame fetch as a second block range: one launch instead of two at the head of every step
            sel = self.opt._sched[0][1]
            rc = lib.bnerv_ctx_wplan_run_fetch(c.handle, L.stream(), L.ptr(self._clip), L.ptr(self._clip_norms), sel.data_ptr() + 5 * 4, self._clip.shape[0],
                                               self._clip[0].numel(), L.ptr(self.static_img), L.ptr(self.static_idx))
            if rc == 0:
                fetched = True
            elif rc != 1:
                L.check(rc, "bnerv_ctx_wplan_run_fetch")
        if not fetched:
            L.check(lib.bnerv_ctx_wplan_run(c.handle, L.stream()), "bnerv_ctx_wplan_run")
        try:
            self._fetch_done = fetched
            self._fwd_bwd()
        finally:
            self._fetch_done = False
            lib.bnerv_ctx_wplan_end(c.handle)

    def _record_wplan(self):
        """One forward + backward on the capture stream, eager, with the stream context recording which weight tensors the wide split
        convs split (gradients are discarded: the next _fwd_bwd starts with zero_grad; no parameter or optimizer state changes).
        Only the plain step: a step whose forward draws random numbers (CompressionStep) would advance its generator here."""
        import os
        from . import _lib as L
        self._wplan_entries = 0
        if type(self) is not TrainStep or os.environ.get("BNERV_WPLAN", "1") == "0":
            return
        # the recording pass is one extra forward + backward: with BatchNorm it would move the running statistics once more than the
        # eager / reference trajectory does, with an active Dropout it would advance the generator -- no plan for such models
        for mod in self.model.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) or (isinstance(mod, torch.nn.modules.dropout._DropoutNd) and mod.p > 0):
                return
        lib = L.load()
        with torch.cuda.stream(self._cap_stream), L.use_ctx(self._cap_ctx) as c:
            L.check(lib.bnerv_ctx_wplan_record(c.handle), "bnerv_ctx_wplan_record")
            early_ok, self._early_ok = self._early_ok, False     # (the recording pass exchanges nothing)
            try:
                self._fwd_bwd()
            finally:
                self._early_ok = early_ok
                n = lib.bnerv_ctx_wplan_freeze(c.handle)
            if n < 0:
                L.check(n, "bnerv_ctx_wplan_freeze")
            self._wplan_entries = n
        self.opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()

    def _dp_hook(self, grad):
        """Autograd hook on the stem output (two buckets): the decoder layers' gradients are complete once their deferred slab reductions
        have run -- flush them, then start the early segment's all-reduce."""
        if self._early_ok:
            from . import ops
            ops._flush_deferred()
            self.bucket.exchange_early()
        return None

    def _eager(self, prepared=False):
        self._fwd_bwd()
        if self.bucket is not None:
            self.bucket.finish()
        self._clip_grads()
        if not prepared:
            self.opt.prepare_step()
        self.opt.launch_step()

    def _clip_grads(self):
        """--clip_max_norm: clip_grad_norm_ of train_nerv_all.py:346-347 on the device (two launches over the optimizer's table, no host round
        trip), after the exchange: the ranks clip the AVERAGED gradient, as DDP followed by clip_grad_norm_ does in the reference.
        With a Pruner the gradient mask comes first (one launch over the same table): the clip sees the norm of the masked gradient."""
        if self.prune is not None:
            self.opt.launch_grad_mask()
        if self.clip_max_norm > 0:
            self.opt.launch_clip(self.clip_max_norm)

    def _bucket_calls(self, which):
        import ctypes as C
        from . import _lib as L
        lib = L.load()
        fn, scale = (lib.bnerv_bucket_gather, 1.0 / self.world) if which == "gather" else (lib.bnerv_bucket_scatter, 1.0)
        for ck in self.bucket._build():
            L.check(fn(L.stream(), C.byref(ck), L.ptr(self.bucket.bucket), scale), "bnerv_bucket_" + which)

    def _capture(self):
        """world == 1: one graph.  world > 1 on RCCL: ONE graph as well -- the all-reduce of the flat bucket is captured between the
        gather and the scatter, so a step is a single launch with no host round trip around the collective (BNERV_DP_INGRAPH=0, a
        backend whose collectives cannot be captured (gloo), or a failed capture fall back to graph A -> eager all-reduce -> graph B)."""
        import os
        import torch.distributed as dist
        from . import _lib as L
        torch.cuda.synchronize()
        self._opt_epoch = getattr(self.opt, "state_epoch", 0)
        pool = torch.cuda.graph_pool_handle()
        self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), None
        # capture on a stream of our own with a library context of our own, whose scratch is reserved BEFORE the capture starts
        # (nothing may allocate inside it; the eager warm-up steps on the current stream sized the scratch)
        if getattr(self, "_cap_stream", None) is None:
            self._cap_stream = torch.cuda.Stream(device=self.dev)
            self._cap_ctx = L.new_ctx()
        else:
            L.reserve_ctx(self._cap_ctx)
        if hasattr(self.opt, "begin_capture"):
            # this capture's own descriptor tables (optimizer._FusedTableOptimizer._table, capture contract) and, with a clip, its workspace
            self.opt.begin_capture(clip=self.clip_max_norm > 0)
        try:
            with L.use_ctx(self._cap_ctx):
                self._capture_in_ctx(pool)
        finally:
            if hasattr(self.opt, "finish_capture"):
                # uploaded once, outside the graph; the tables live as long as this object's graphs
                self._opt_tables = self.opt.finish_capture()

    def _capture_in_ctx(self, pool):
        import os
        import torch.distributed as dist
        from . import _lib as L
        self._early_ok = False
        self._record_wplan()
        self._early_ok = True
        cap = dict(pool=pool, stream=self._cap_stream)
        if self.bucket is None:
            with L.graph_capture(self.graph_a, **cap):
                self._planned_fwd_bwd()
                self._clip_grads()
                self.opt.launch_step()
            return

        def head():
            self._planned_fwd_bwd()
            for p in self.params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            self._bucket_calls("gather")

        def tail():
            self._bucket_calls("scatter")
            self._clip_grads()
            self.opt.launch_step()
        backend = dist.get_backend(self.bucket.group) if dist.is_initialized() else ""
        if backend == "nccl" and os.environ.get("BNERV_DP_INGRAPH", "1") != "0":
            try:
                with L.graph_capture(self.graph_a, **cap):
                    self._planned_fwd_bwd()                   # (two buckets: the hook starts the early segment's all-reduce in here)
                    self.bucket.finish()                      # gather -> all-reduce -> [join] -> scatter
                    self._clip_grads()
                    self.opt.launch_step()
                self.collective_in_graph = True
                return
            except Exception as e:                        # capture of the collective is not available on this stack: two graphs
                import warnings
                warnings.warn(f"RCCL all-reduce could not be captured ({type(e).__name__}: {e}); falling back to the two-graph step")
                torch.cuda.synchronize()
                self.graph_a = torch.cuda.CUDAGraph()
        self.collective_in_graph = False
        self._early_ok = False                              # graph A cannot hold a collective: one exchange between the two graphs
        self.bucket._early_inflight = False
        self.bucket._side_used = None
        with L.graph_capture(self.graph_a, **cap):
            head()
        self.graph_b = torch.cuda.CUDAGraph()
        with L.graph_capture(self.graph_b, **cap):
            tail()

    # ---- one step ------------------------------------------------------------------------------------------------------
    def __call__(self, img, norm_idx, frame_idx=None):
        """img [B,3,H,W] fp32 and norm_idx [B] fp64, already on the device.  Returns (loss, psnr[B]) device tensors that are
        overwritten by the next call.  frame_idx [B] (any number type, on the device): with a YuvTerm, the raw frames img was made of."""
        if self._fetching:
            self._fetching = False
            self.graph_a = self.graph_b = None      # the captured step started with a frame fetch: capture the plain form
        self.static_img.copy_(img, non_blocking=True)
        self.static_idx.copy_(norm_idx, non_blocking=True)
        if self.yuv is not None:
            if frame_idx is None:
                raise ValueError("TrainStep: a step with the plane loss needs frame_idx, the numbers of the raw frames to compare against")
            self.yuv_sel.copy_(frame_idx.reshape(-1), non_blocking=True)
        return self._run(None)

    def step_frame(self, i):
        """Train frame i of the clip given to bind_clip().  Same step as __call__(frames[i:i+1], norms[i:i+1])."""
        assert self._clip is not None, "step_frame: call bind_clip(frames, norms) first"
        i = int(i)
        if not 0 <= i < self._clip.shape[0]:    # (the fetch kernel clamps the index it reads from the schedule record: never hand it a bad one)
            raise IndexError(f"step_frame: frame {i} outside the bound clip of {self._clip.shape[0]} frames")
        if not self._fetching:
            self._fetching = True
            self.graph_a = self.graph_b = None
        return self._run(int(i))

    def _run(self, frame):
        if self.graph_a is not None and getattr(self.opt, "state_epoch", 0) != self._opt_epoch:
            self.graph_a = self.graph_b = None      # optimizer state tensors were replaced (restart_opt / load_state_dict): re-capture
        if frame is not None:
            self.opt.prepare_step(aux=frame)    # the schedule record (with the frame index) precedes the step's first launch
        if not self.use_graph or self.n_calls < self.warmup_eager:
            self._eager(prepared=frame is not None)
        else:
            if frame is None:
                self.opt.prepare_step()         # host side of THIS step (a capture below records its kernels, runs nothing)
            if self.graph_a is None:
                self._capture()
            self.graph_a.replay()
            if self.graph_b is not None:
                import torch.distributed as dist
                dist.all_reduce(self.bucket.bucket, op=dist.ReduceOp.SUM, group=self.bucket.group)
                self.graph_b.replay()
        self.n_calls += 1
        return self.loss_out, self.psnr_out


class CompressionStep(TrainStep):
    """The rate-distortion step of train_nerv_compression.py:354-367 (quantise + rate term over all tensors -> forward with the
    embedding's rate -> loss + lambda * bpp while bpp / N exceeds the target -> backward -> Adan) as ONE captured graph.  The
    `bpp > target` decision is a device-side gate and the training noise comes from the capture-aware default generator, so
    nothing in the step needs the host.  With several ranks the quantiser / rate parameters are part of the same flat gradient
    bucket as the weights (they are model parameters), exchanged exactly as in TrainStep.  Returns (final_loss, psnr[B]);
    `bpp_out` holds bits per pixel (x N)."""

    def __init__(self, model, optimizer, entropy_model, args, batch_shape, device, use_graph=True, warmup_eager=3, world_size=1,
                 process_group=None, force_bucket=False, prune=None, yuv=None):
        if prune is not None:
            raise NotImplementedError("CompressionStep: pruning is built for the plain train step only (engine.TrainStep)")
        super().__init__(model, optimizer, args.loss, "HNeRV_Boost" in args.model or 'pe' not in args.embed, batch_shape, device,
                         use_graph=use_graph, warmup_eager=warmup_eager, clip_max_norm=getattr(args, "clip_max_norm", 0.0),
                         world_size=world_size, process_group=process_group, force_bucket=force_bucket, yuv=yuv)
        self.entropy_model, self.cargs = entropy_model, args
        self.bpp_out = None

    def _fwd_bwd(self):
        a, m = self.cargs, self.model
        if self._fetching:
            self._fetch()                       # bind_clip() / step_frame(): the step starts with the frame fetch, as TrainStep's does
        self.opt.zero_grad(set_to_none=True)
        m.cal_params(self.entropy_model)
        inp = self.static_img if self.takes_image else self.static_idx
        if a.embed_entropy:
            img_out, _, _ = m(inp, entropy_model=self.entropy_model, norm_idx=self.static_idx)
            bpp = (m.get_bitrate_sum(name="bitrate") + m.bitrate_e_dict["bitrate"] * a.full_data_length) / a.final_size
        else:
            img_out, _, _ = m(inp, norm_idx=self.static_idx)
            bpp = m.get_bitrate_sum(name="bitrate") / a.final_size
        if self.yuv is None:
            out_loss = hu.loss_fn(img_out, self.static_img, self.loss_type)
        else:                                   # the plane loss through its autograd form, added to (or, pure, in place of) the RGB loss
            y = self.yuv
            if y.lam_ms > 0:
                term, self.yuv_stats_out, self.yuv_ms_out = y.autograd_term(img_out, self._yuv_sel())
                out_loss = term if y.pure else hu.loss_fn(img_out, self.static_img, self.loss_type) + term
            else:
                term, self.yuv_stats_out = y.loss(img_out, self._yuv_sel())
                out_loss = y.lam * term if y.pure else hu.loss_fn(img_out, self.static_img, self.loss_type) + y.lam * term
        gate = (bpp.detach() / a.full_data_length > a.target_bpp).to(out_loss.dtype)     # `if bpp / N > target_bpp` (:363) on the device
        final_loss = out_loss + gate * a.lambda_rate * bpp
        final_loss.backward()
        self.loss_out = final_loss.detach()
        self.bpp_out = bpp.detach()
        self.psnr_out = ops.psnr(img_out.detach(), self.static_img)

    def _capture(self):
        # The model's rate dictionaries and dequantised tensors still reference the autograd graph of the last eager step; that
        # keeps its AccumulateGrad nodes (created on the default stream) alive, the capture would reuse them and pull the
        # default stream into the capture (hipStreamEndCapture crashes on it).  Detach every such reference first.
        for mod in self.model.modules():
            for k, v in list(vars(mod).items()):
                if torch.is_tensor(v) and v.grad_fn is not None:
                    setattr(mod, k, v.detach())
                elif isinstance(v, dict) and not k.startswith("_"):
                    for kk, vv in list(v.items()):
                        if torch.is_tensor(vv) and vv.grad_fn is not None:
                            v[kk] = vv.detach()
        super()._capture()


class DecodeGraph:
    """Forward-only decode of one batch as a captured hipGraph (row N4: the rate evaluate() logs as "FPS" under --eval_fps,
    train_nerv_all.py:492-496 of the reference, is ~35 Python-driven launches per frame when run eagerly).  The graph replays
    `model(cur_input, embed, norm_idx=norm_idx)` on static copies of its inputs; `__call__` refreshes them, replays, and returns
    (img_out, seconds) with the same synchronised-timer definition the model's own `dec_time` uses."""

    def __init__(self, model, cur_input, embed, norm_idx):
        import time as _time
        self._time = _time
        self.inp = cur_input.clone()
        self.embed = None if embed is None else embed.clone()
        self.norm = norm_idx.clone()
        td = getattr(model, "time_decode", False)
        model.time_decode = False                           # no host synchronisation inside the capture
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        import os
        from . import _lib as L
        lib = L.load()
        self._ctx = L.new_ctx()
        plan = os.environ.get("BNERV_WPLAN", "1") != "0"
        try:
            with torch.no_grad(), torch.cuda.stream(side), L.use_ctx(self._ctx) as c:
                # warm-up: workspaces and lazily built tables exist before capture; the first one records which weight tensors the
                # wide split convs split.  A decoder's weights are fixed, so their 16-bit fragments are prepared ONCE, here
                # (bnerv_ctx_wplan_*), and the captured forward launches no preparation at all; refresh() after a weight change.
                if plan:
                    L.check(lib.bnerv_ctx_wplan_record(c.handle), "bnerv_ctx_wplan_record")
                model(self.inp, self.embed, norm_idx=self.norm)
                self.wplan_entries = lib.bnerv_ctx_wplan_freeze(c.handle) if plan else 0
                if self.wplan_entries < 0:
                    L.check(self.wplan_entries, "bnerv_ctx_wplan_freeze")
                model(self.inp, self.embed, norm_idx=self.norm)
                L.check(lib.bnerv_ctx_wplan_run(c.handle, L.stream()), "bnerv_ctx_wplan_run")
                try:
                    self.graph = torch.cuda.CUDAGraph()
                    with L.graph_capture(self.graph, stream=side):
                        self.out = model(self.inp, self.embed, norm_idx=self.norm)[0]
                finally:
                    lib.bnerv_ctx_wplan_end(c.handle)
        finally:
            model.time_decode = td
            cur.wait_stream(side)

    def refresh(self):
        """Re-prepare the weight fragments the captured forward reads (one launch) after the model's weights were written."""
        from . import _lib as L
        L.check(L.load().bnerv_ctx_wplan_run(self._ctx.handle, L.stream()), "bnerv_ctx_wplan_run")
        L.load().bnerv_ctx_wplan_end(self._ctx.handle)

    def matches(self, cur_input, embed, norm_idx):
        return (cur_input.shape == self.inp.shape and norm_idx.shape == self.norm.shape and
                (embed is None) == (self.embed is None) and (embed is None or embed.shape == self.embed.shape))

    def __call__(self, cur_input, embed, norm_idx):
        self.inp.copy_(cur_input)
        self.norm.copy_(norm_idx)
        if self.embed is not None:
            self.embed.copy_(embed)
        torch.cuda.synchronize()
        t0 = self._time.time()
        self.graph.replay()
        torch.cuda.synchronize()
        return self.out, self._time.time() - t0


class _ForwardAndPack:
    """What FrameDecodeGraph captures: the model's forward followed by the packing kernel into a static frame buffer -- uint8 RGB
    (coeffs None) or raw YUV 4:2:0 in file layout (coeffs: yuvio.coefficients of the pixel format).  up = (size, scratch, full): the frame is
    up-sampled to `size` on the way -- ops.resize_to_yuv420 in place of the store kernel, or ops.resize_bicubic into the
    static fp32 frame `full` in front of ops.frame_to_u8."""
    time_decode = False

    def __init__(self, model, packed, coeffs=None, up=None):
        self.model, self.packed, self.coeffs, self.up = model, packed, coeffs, up

    def __call__(self, cur_input, embed, norm_idx=None):
        from . import ops
        out = self.model(cur_input, embed, norm_idx=norm_idx)[0]
        if self.up is not None:
            size, scratch, full = self.up
            if self.coeffs is None:
                ops.frame_to_u8(ops.resize_bicubic(out, size, out=full, scratch=scratch), out=self.packed)
            else:
                ops.resize_to_yuv420(out, size, self.coeffs, out=self.packed, scratch=scratch)
        elif self.coeffs is None:
            ops.frame_to_u8(out, out=self.packed)
        else:
            ops.rgb_to_yuv420(out, self.coeffs, out=self.packed)
        return (out,)


class FrameDecodeGraph:
    """The frame loop of a bitstream decoder (codec.Decoder): DecodeGraph's capture -- same warm-up, same weight-fragment plan -- of the
    forward PLUS ops.frame_to_u8, replayed WITHOUT a host synchronisation.  `launch(cur_input, embed, norm_idx)` refreshes the static inputs
    with device-side copies and replays on the current stream; `out` ([B, 3, H, W] fp32) and `u8` ([B, H, W, 3] uint8) are the static results,
    valid in stream order until the next launch.  use_graph=False runs the same two steps eagerly into the same buffers.
    pack selects the packing node behind the forward: "rgb8" (ops.frame_to_u8), or "yuv420p" / "yuv420p10le" (ops.rgb_to_yuv420 with the
    given matrix and range; `u8` is then [B, frame bytes] uint8, every frame in file layout: planes Y, U, V).
    upscale=(H, W) packs the frame up-sampled to H x W: `out` stays the model's frame of frame_hw, `u8` and `out_hw` are
    of the up-sampled size; the pack node is ops.resize_to_yuv420, or ops.resize_bicubic + ops.frame_to_u8 for "rgb8".  Its buffers (the row
    pass's scratch, for "rgb8" the full-size fp32 frame) are allocated here, once, and its tables uploaded before the capture."""

    def __init__(self, model, cur_input, embed, norm_idx, frame_hw, use_graph=True, pack="rgb8", matrix="bt709", range="limited", upscale=None):
        self.use_graph, self.pack = use_graph, pack
        dev = norm_idx.device
        B, (H, W) = norm_idx.shape[0], frame_hw
        if upscale is not None:
            H, W = (int(v) for v in upscale)
            if H < 1 or W < 1:
                raise ValueError(f"FrameDecodeGraph: upscale={tuple(upscale)}")
        self.out_hw = (H, W)
        if pack == "rgb8":
            self.coeffs = None
            self.u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        else:
            from . import yuvio
            if pack not in yuvio.PIX_FMTS:
                raise ValueError(f"FrameDecodeGraph: pack={pack!r} (rgb8, {', '.join(yuvio.PIX_FMTS)})")
            if H % 2 or W % 2:
                raise ValueError(f"FrameDecodeGraph: 4:2:0 needs even dimensions, the frames are {H}x{W}")
            self.coeffs = yuvio.coefficients(matrix, range, yuvio.PIX_FMTS[pack])
            self.u8 = torch.empty(B, yuvio.frame_samples(H, W) * self.coeffs.bytes_per_sample, dtype=torch.uint8, device=dev)
        up = None
        if upscale is not None:
            from . import ops
            ops._resize_table(frame_hw[1], W, dev)          # (the tap limit is refused here; the uploads precede the capture)
            ops._resize_table(frame_hw[0], H, dev)
            up = ((H, W), torch.empty(B * 3 * frame_hw[0] * W, dtype=torch.float32, device=dev),
                  torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if self.coeffs is None else None)
        self._body = _ForwardAndPack(model, self.u8, self.coeffs, up)
        td = getattr(model, "time_decode", False)
        model.time_decode = False
        try:
            if use_graph:
                self._dg = DecodeGraph(self._body, cur_input, embed, norm_idx)
                self.inp, self.embed, self.norm, self.out = self._dg.inp, self._dg.embed, self._dg.norm, self._dg.out
                torch.cuda.current_stream().synchronize()
            else:
                self._dg = None
                self.inp, self.embed, self.norm = cur_input.clone(), None if embed is None else embed.clone(), norm_idx.clone()
                with torch.no_grad():
                    self.out = self._body(self.inp, self.embed, norm_idx=self.norm)[0]
        finally:
            model.time_decode = td
        if tuple(self.out.shape[-2:]) != tuple(frame_hw):
            raise ValueError(f"FrameDecodeGraph: the model decodes {tuple(self.out.shape[-2:])} frames, the caller announced {tuple(frame_hw)}")

    def launch(self, cur_input, embed, norm_idx):
        self.inp.copy_(cur_input, non_blocking=True)
        self.norm.copy_(norm_idx, non_blocking=True)
        if self.embed is not None:
            self.embed.copy_(embed, non_blocking=True)
        if self._dg is not None:
            self._dg.graph.replay()
        else:
            with torch.no_grad():
                self.out = self._body(self.inp, self.embed, norm_idx=self.norm)[0]
        return self.out, self.u8
