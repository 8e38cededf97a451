"""Adan optimizer -- host-side mirror of the reference's optimizer.py:39-235 (same constructor signature, defaults,
param_group / state key names: 'step', 'exp_avg', 'exp_avg_sq', 'exp_avg_diff', 'neg_pre_grad'), with the update itself
done by ONE fused multi-tensor HIP kernel per <=48 tensors (bnerv_adan_multi_tensor) instead of ~17 torch._foreach
launches (optimizer.py:296-362).  This is the slot the reference reserves for the external `fused_adan` CUDA extension
(optimizer.py:365-395), which it never ships.

`step()` = `prepare_step()` (host: step count, bias corrections, lr -> an 8-float device buffer, via a pinned async copy)
+ `launch_step()` (kernel launches only -> capturable in a hipGraph; every scalar that changes per step is read from the
device buffer, so a captured step replays with a moving LR schedule)."""
import ctypes as C
import math

import torch
from torch.optim.optimizer import Optimizer

from . import _lib as L


class _FusedTableOptimizer(Optimizer):
    """The driver the fused optimizers share: the device schedule record written by prepare_step(), the device-resident descriptor table
    of launch_step() and its capture bracket.  A subclass supplies the record's values (_sched_record), the per-parameter state
    (_ensure_state), the state tensors of a table entry (_entry_state) and the launch (_launch)."""
    _RING = 512

    def _init_driver(self):
        self._sched = {}          # group index -> (pinned host [5], device [5])
        self._cap_open = None     # begin_capture() .. finish_capture(): group index -> (pinned host, device) descriptor table of THIS capture
        self._chunk_cache = {}    # group index -> (key, device descriptor table, n, blocks, tensors the table points into, pending host table)
        self.state_epoch = 0      # bumped whenever state tensors are replaced: a captured step (engine.TrainStep) re-captures
        self._clip_ws = None      # launch_clip(): one double per block of every group's table (device)
        self.clip_out = None      # launch_clip(): device [2] = (total gradient norm, clip coefficient) of the last clip
        self._grad_masks = None   # set_grad_masks(): parameter -> uint8 mask (prune.Pruner); the tables then carry a mask pointer per entry
        self._mask_late = []      # launch_grad_mask() -> launch_clip(): parameters whose state was made from the unclipped gradient

    def _invalidate(self):
        """The descriptors of launch_step() hold raw device pointers into the state tensors; whoever replaces those tensors
        (restart_opt, load_state_dict, unpickling) must drop the descriptors, and a captured graph of the step with them."""
        self._chunk_cache = {}
        self.state_epoch = getattr(self, "state_epoch", 0) + 1

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._invalidate()

    def _clip_coef(self):
        return 1.0

    def set_grad_masks(self, masks):
        """masks: {parameter: uint8 tensor of its shape} (None: no masks).  From now on every descriptor table is followed, in the same
        buffer, by one mask pointer per entry (NULL for a parameter without a mask) -- what launch_grad_mask() reads.  The masks keep
        their addresses for the life of the optimizer's tables (prune.Pruner allocates them once)."""
        self._grad_masks = None if not masks else {id(p): m for p, m in masks.items()}
        self._chunk_cache = {}

    def _clip_fresh(self, group):
        """launch_clip(): the parameters of `group` whose state the table is about to create from the UNCLIPPED gradient."""
        return []

    @torch.no_grad()
    def prepare_step(self, aux=None):
        """Host side of a step: advance the step count and publish the schedule record (_sched_record: lr and bias corrections, slots 0..4) and aux to the device.
        `aux` (a float, optional) rides in slot 5 of the same 32-byte record: engine.TrainStep puts the index of the step's frame
        there when the clip is resident on the device, so a step costs ONE host -> device copy."""
        for gi, group in enumerate(self.param_groups):
            group["step"] = group.get("step", 0) + 1
            dev = group["params"][0].device
            L.require_device(group["params"][0], "parameter")
            if gi not in self._sched:
                # a RING of pinned slots: the async copy of step k may still be queued when the host prepares step k+1.  Every slot
                # carries an event recorded after its copy was enqueued; a slot is rewritten only once that copy has executed, which
                # bounds the host's run-ahead to _RING steps by construction (in practice the HIP launch queue already blocks the host
                # long before 512 graph launches are outstanding; the guard makes that an invariant instead of an observation)
                self._sched[gi] = (torch.zeros(self._RING, 8, dtype=torch.float32).pin_memory(), torch.zeros(8, dtype=torch.float32, device=dev),
                                   [None] * self._RING)
            ring, devbuf, events = self._sched[gi]
            slot = group["step"] % self._RING
            if events[slot] is not None:
                events[slot].synchronize()
            host = ring[slot]
            rec = self._sched_record(group)
            for i, v in enumerate(rec):
                host[i] = v
            if aux is not None:
                host[5] = float(aux)
            devbuf.copy_(host, non_blocking=True)
            if events[slot] is None:
                events[slot] = torch.cuda.Event()
            events[slot].record()

    def _table(self, lib, gi, group, clip, what):
        """The device-resident descriptor table of group gi for the gradients that exist now -- built, or refreshed when a tensor address
        changed, and uploaded (outside a capture).  -> (device table, tensors, blocks), None for a group without gradients.  launch_clip()
        and launch_step() of one step share it: the second call finds the first one's table.

        Capture contract: a captured launch records only the ADDRESS of its descriptor table; the content is uploaded by
        finish_capture().  Inside a stream capture this method therefore raises unless a begin_capture() .. finish_capture() bracket
        is open (engine.TrainStep._capture opens one); every bracket gets a table of its own, which the caller keeps alive with its
        graph (finish_capture() returns it), so a second capture never rewrites the table an earlier graph still replays with."""
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return None
        # the key covers every pointer a descriptor holds (parameter, gradient and the four state tensors), and the cache
        # entry keeps the state tensors alive, so a descriptor can never point at freed memory
        sts = [self._ensure_state(p, group.get("step", 1), clip) for p in ps]
        ents = [self._entry_state(st) for st in sts]          # (exp_avg, exp_avg_sq, exp_avg_diff | None, neg_pre_grad | None)
        key = tuple((p.data_ptr(), p.grad.data_ptr()) + tuple(0 if t is None else t.data_ptr() for t in en) for p, en in zip(ps, ents))
        gm = getattr(self, "_grad_masks", None)
        if gm is not None:
            mptr = [gm[id(p)].data_ptr() if id(p) in gm else 0 for p in ps]
            key += (tuple(mptr),)
        capturing = torch.cuda.is_current_stream_capturing()
        ck = (gi, capturing)        # a captured launch owns its table: an eager step in between must not rewrite the addresses it replays with
        if capturing and self._cap_open is None:
            raise L.BnervError(f"{type(self).__name__}.{what}() inside a stream capture needs an open begin_capture() .. finish_capture() bracket "
                               "(the captured launch reads a descriptor table that finish_capture() uploads)")
        cached = self._chunk_cache.get(ck)
        if capturing and cached is not None and cached[1] is not self._cap_open[gi][1]:
            cached = None               # a table of an earlier capture: that graph keeps it; this capture writes its own
        if cached is None or cached[0] != key:
            # (not p.grad: it is alive whenever the step launches, and pinning it would move the next eager gradient elsewhere)
            keep = [(p,) + tuple(en) for p, en in zip(ps, ents)] + ([] if gm is None else [gm[id(p)] for p in ps if id(p) in gm])
            tab = (L.AdanEntry * len(ps))()
            blocks = 0
            for j, (p, en) in enumerate(zip(ps, ents)):
                if not (p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32 and p.grad.dtype == torch.float32):
                    raise L.BnervError(f"fused {type(self).__name__} needs contiguous fp32 parameters and gradients")
                e = tab[j]
                e.p, e.g = p.data_ptr(), p.grad.data_ptr()
                e.exp_avg, e.exp_avg_sq = en[0].data_ptr(), en[1].data_ptr()
                e.exp_avg_diff = None if en[2] is None else en[2].data_ptr()
                e.neg_pre_grad = None if en[3] is None else en[3].data_ptr()
                e.n, e.bstart = p.numel(), blocks
                blocks += lib.bnerv_adan_table_blocks(p.numel())
            raw = bytes(tab)
            if gm is not None:              # the mask pointers of the entries, behind the table (launch_grad_mask)
                raw += bytes((C.c_uint64 * len(ps))(*mptr))
            if capturing:
                # nothing may allocate pinned or device memory inside a capture: begin_capture() set both aside
                host, dev_tab = self._cap_open[gi]
                if host.numel() < len(raw):
                    raise L.BnervError("fused optimizer: the capture-time descriptor table is larger than the one begin_capture() reserved")
                C.memmove(host.data_ptr(), raw, len(raw))
            else:
                host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
                # ONE device table per group, reused while the tensor count does not change
                dev_tab = cached[1] if (cached is not None and cached[1].numel() == host.numel()) else torch.empty(host.numel(), dtype=torch.uint8, device=ps[0].device)
            cached = [key, dev_tab, len(ps), blocks, keep, host]
            self._chunk_cache[ck] = cached
        if cached[5] is not None and not capturing:
            cached[1].copy_(cached[5], non_blocking=True)      # stream-ordered before the launch that follows
            cached[5] = None                                   # (inside a capture the upload waits for finish_capture(): a copy node would replay every step)
        return cached[1], cached[2], cached[3]

    @torch.no_grad()
    def launch_step(self, clip=1.0):
        """Device side of a step: ONE fused launch over a device-resident descriptor table (any number of tensors).  No sync; the
        only host<->device traffic is the table upload when a tensor address changed (never in a replayed step).  Inside a stream
        capture: see the capture contract of _table()."""
        lib = L.load()
        for gi, group in enumerate(self.param_groups):
            tab = self._table(lib, gi, group, clip, "launch_step")
            if tab is not None:
                self._launch(lib, group, clip, self._sched[gi][1].data_ptr(), tab[0].data_ptr(), tab[1], tab[2])

    def _clip_buffers(self):
        """The clip's workspace (one double per block the tables of ALL parameters can have) and its 2-float result, made once: on the first
        eager launch_clip(), or by begin_capture(clip=True) when a capture comes first."""
        lib = L.load()
        need = sum(lib.bnerv_adan_table_blocks(p.numel()) for group in self.param_groups for p in group["params"])
        if self._clip_ws is None or self._clip_ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise L.BnervError("fused optimizer: launch_clip() inside a stream capture needs the workspace begin_capture(clip=True) reserves")
            dev = self.param_groups[0]["params"][0].device
            self._clip_ws = torch.zeros(max(need, 1), dtype=torch.float64, device=dev)
            if self.clip_out is None:
                self.clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
        return self._clip_ws, self.clip_out

    @torch.no_grad()
    def launch_clip(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) on the device, in front of launch_step(): two launches per parameter group
        over launch_step()'s own descriptor table (bnerv_grad_sqsum_table, bnerv_grad_scale_table), no host round trip -- capturable under
        launch_step()'s capture contract.  The norm is global: every group's partial sums go into one workspace and every group is scaled
        by the sum of all of them.  `clip_out` (device, [2]) then holds (total norm, coefficient)."""
        lib = L.load()
        ws, out = self._clip_buffers()
        tabs, late, base = [], [], 0
        for gi, group in enumerate(self.param_groups):
            fresh = self._clip_fresh(group)
            tab = self._table(lib, gi, group, 1.0, "launch_clip")
            if tab is None:
                continue
            late += fresh
            tabs.append((tab, base))
            L.check(lib.bnerv_grad_sqsum_table(L.stream(), tab[0].data_ptr(), tab[1], tab[2], ws.data_ptr() + 8 * base), "bnerv_grad_sqsum_table")
            base += tab[2]
        late += self._mask_late             # (launch_grad_mask() of this step met them first: their state exists by now)
        self._mask_late = []
        for tab, _ in tabs:
            L.check(lib.bnerv_grad_scale_table(L.stream(), tab[0].data_ptr(), tab[1], tab[2], ws.data_ptr(), base, float(max_norm), out.data_ptr()),
                    "bnerv_grad_scale_table")
        for p in late:                      # (their state was made from the gradient as it was BEFORE the clip)
            self.state[p]["neg_pre_grad"].copy_(p.grad).neg_()

    @torch.no_grad()
    def launch_grad_mask(self):
        """p.grad *= mask for every parameter that has one (set_grad_masks), ONE launch per parameter group over launch_step()'s own
        descriptor table (bnerv_grad_mask_table) -- capturable under launch_step()'s capture contract.  In front of launch_clip() and
        launch_step(): the clip then sees the masked norm and the update a zero gradient wherever a weight is pruned."""
        if getattr(self, "_grad_masks", None) is None:
            raise L.BnervError("fused optimizer: launch_grad_mask() without set_grad_masks()")
        lib = L.load()
        for gi, group in enumerate(self.param_groups):
            fresh = self._clip_fresh(group)
            tab = self._table(lib, gi, group, 1.0, "launch_grad_mask")
            if tab is None:
                continue
            L.check(lib.bnerv_grad_mask_table(L.stream(), tab[0].data_ptr(), tab[1], tab[2], tab[0].data_ptr() + tab[1] * C.sizeof(L.AdanEntry)),
                    "bnerv_grad_mask_table")
            for p in fresh:                 # (their state was made from the gradient as it was BEFORE the mask; a clip that follows redoes this)
                self.state[p]["neg_pre_grad"].copy_(p.grad).neg_()
            self._mask_late += fresh

    def begin_capture(self, clip=False):
        """Before a hipGraph capture that will contain launch_step(): reserve THIS capture's descriptor tables (pinned host + device,
        one pair per parameter group, sized for every parameter) -- nothing may allocate inside the capture.  clip: the capture will
        contain launch_clip() as well, whose workspace and result are made here unless an eager launch_clip() already made them."""
        tabs = {}
        for gi, group in enumerate(self.param_groups):
            nb = max(len(group["params"]), 1) * (C.sizeof(L.AdanEntry) + (8 if getattr(self, "_grad_masks", None) is not None else 0))
            dev = group["params"][0].device
            host = torch.empty(nb, dtype=torch.uint8)
            tabs[gi] = (host.pin_memory() if dev.type == "cuda" else host, torch.empty(nb, dtype=torch.uint8, device=dev))
        self._cap_open = tabs
        if clip:
            self._clip_buffers()

    def finish_capture(self):
        """After a hipGraph capture that contained launch_step(): upload the descriptor tables that capture referenced (the captured
        launch holds the table's ADDRESS; its content is written here, once, outside the graph) and close the bracket.  Returns the
        device tables: the owner of the graph keeps them alive as long as the graph."""
        for cached in self._chunk_cache.values():
            if cached[5] is not None:
                cached[1].copy_(cached[5], non_blocking=True)
                torch.cuda.current_stream().synchronize()          # the pinned buffer dies with the bracket
                cached[5] = None
        tabs, self._cap_open = self._cap_open, None
        return [] if tabs is None else [t[1] for t in tabs.values()]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self._clip_coef()
        self.prepare_step()
        self.launch_step(clip)
        return loss


class Adan(_FusedTableOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0,
                 no_prox=False, foreach: bool = True, fused: bool = False):
        if not 0.0 <= max_grad_norm:
            raise ValueError("Invalid Max grad norm: {}".format(max_grad_norm))
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        for i in range(3):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError("Invalid beta parameter at index {}: {}".format(i, betas[i]))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, no_prox=no_prox,
                        foreach=foreach, fused=fused)
        super().__init__(params, defaults)
        self._init_driver()

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("no_prox", False)
        self.__dict__.setdefault("_sched", {})
        self.__dict__["_cap_open"] = None
        self.__dict__.setdefault("_clip_ws", None)
        self.__dict__.setdefault("clip_out", None)
        self.__dict__["_grad_masks"] = None         # (keyed by parameter identity: a copy has none until a Pruner is attached to it)
        self.__dict__["_mask_late"] = []
        self._invalidate()

    @torch.no_grad()
    def restart_opt(self):
        for group in self.param_groups:
            group["step"] = 0
            for p in group["params"]:
                if p.requires_grad:
                    state = self.state[p]
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                    state["exp_avg_diff"] = torch.zeros_like(p)
        self._invalidate()

    # ------------------------------------------------------------------------------------------------------------------
    def _clip_coef(self):
        if self.defaults["max_grad_norm"] <= 0:
            return 1.0
        # optimizer.py:136-156: global-norm clipping (a device sync, exactly as in the reference; off in every recipe)
        device = self.param_groups[0]["params"][0].device
        total = torch.zeros(1, device=device)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    total.add_(p.grad.pow(2).sum())
        total = torch.sqrt(total)
        return torch.clamp(self.defaults["max_grad_norm"] / (total + self.param_groups[-1]["eps"]), max=1.0).item()

    def _clip_fresh(self, group):
        # a parameter whose first gradient appears after step 1 starts from neg_pre_grad = -(its gradient) (_ensure_state): after the clip
        if group.get("step", 1) <= 1:
            return []
        return [p for p in group["params"] if p.grad is not None and "neg_pre_grad" not in self.state[p]]

    def _sched_record(self, group):
        beta1, beta2, beta3 = group["betas"]
        t = group["step"]
        return (group["lr"], 1.0 - beta1 ** t, 1.0 - beta2 ** t, math.sqrt(1.0 - beta3 ** t), 1.0 if t == 1 else 0.0)

    def _ensure_state(self, p, step, clip):
        state = self.state[p]
        if len(state) == 0:
            state["exp_avg"] = torch.zeros_like(p)
            state["exp_avg_sq"] = torch.zeros_like(p)
            state["exp_avg_diff"] = torch.zeros_like(p)
        if "neg_pre_grad" not in state:
            # step 1: the kernel's first_step flag substitutes -g; later first appearances follow optimizer.py:190-192
            state["neg_pre_grad"] = torch.zeros_like(p) if step <= 1 else p.grad.clone().mul_(-clip)
        return state

    @staticmethod
    def _entry_state(st):
        return st["exp_avg"], st["exp_avg_sq"], st["exp_avg_diff"], st["neg_pre_grad"]

    def _launch(self, lib, group, clip, sched_ptr, table_ptr, n, blocks):
        beta1, beta2, beta3 = group["betas"]
        hyper = L.AdanHyper(beta1, beta2, beta3, group["eps"], group["weight_decay"], clip, int(group["no_prox"]), sched_ptr)
        L.check(lib.bnerv_adan_table(L.stream(), table_ptr, n, blocks, C.byref(hyper)), "bnerv_adan_table")


class Adam(_FusedTableOptimizer):
    """torch.optim.Adam with its defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) as ONE fused launch per step
    (bnerv_adam_table), with the driver interface of Adan -- so engine.TrainStep captures it, and bind_clip() finds the frame index in its
    schedule record.  state_dict() has torch.optim.Adam's layout (per parameter 'step', 'exp_avg', 'exp_avg_sq'), so a checkpoint of the
    reference (`--optim_type Adam`, train_nerv_all.py:250-251) resumes here and the other way round."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        for i in range(2):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError("Invalid beta parameter at index {}: {}".format(i, betas[i]))
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("fused Adam: weight_decay / amsgrad are not on the HIP path (no recipe sets them)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)
        self._init_driver()

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_sched", {})
        self.__dict__["_cap_open"] = None
        self.__dict__.setdefault("_clip_ws", None)
        self.__dict__.setdefault("clip_out", None)
        self.__dict__["_grad_masks"] = None         # (keyed by parameter identity: a copy has none until a Pruner is attached to it)
        self.__dict__["_mask_late"] = []
        self._invalidate()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:                    # the step count lives in the per-parameter state of a torch.optim.Adam checkpoint
            steps = [int(self.state[p]["step"]) for p in group["params"] if "step" in self.state.get(p, {})]
            if steps:
                group["step"] = max(steps)

    def state_dict(self):
        for group in self.param_groups:                    # publish the group's step count where torch.optim.Adam keeps it
            for p in group["params"]:
                if p in self.state and "exp_avg" in self.state[p]:
                    self.state[p]["step"] = torch.tensor(float(group.get("step", 0)))
        sd = super().state_dict()
        for g in sd["param_groups"]:
            g.pop("step", None)
        return sd

    def _sched_record(self, group):
        beta1, beta2 = group["betas"]
        t = group["step"]
        return (group["lr"], 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t), 1.0 - beta1, 1.0 - beta2)

    def _ensure_state(self, p, step, clip):
        state = self.state[p]
        if "exp_avg" not in state:
            state["step"] = torch.tensor(0.0)
            state["exp_avg"] = torch.zeros_like(p)
            state["exp_avg_sq"] = torch.zeros_like(p)
        return state

    @staticmethod
    def _entry_state(st):
        return st["exp_avg"], st["exp_avg_sq"], None, None

    def _launch(self, lib, group, clip, sched_ptr, table_ptr, n, blocks):
        beta1, beta2 = group["betas"]
        hyper = L.AdanHyper(beta1, beta2, 0.0, group["eps"], 0.0, 1.0, 0, sched_ptr)
        L.check(lib.bnerv_adam_table(L.stream(), table_ptr, n, blocks, C.byref(hyper)), "bnerv_adam_table")
