"""Global magnitude pruning with masked fine-tuning: step one of the NeRV-family compression pipeline
(prune -> 8-bit quantisation -> entropy coding), in front of the post-hoc quantisation and the .bnrq file train_nerv_all.py already ends with.

  prunable set P   every parameter with dim() > 1 whose name does not start with `encoder.` (no file stores the encoder)
  event to s       k = int(round(s * n)); tau = k-th smallest |w| over ALL of P (exact); an element is kept iff |w| > tau -- ties at tau are
                   pruned, so the pruned count is >= k.  Weights AND every per-element optimizer state of P are multiplied by the masks.
  every step       engine.TrainStep(prune=...) multiplies the gradients of P by the masks in one launch, in front of clip and update.
  invariant        a pruned weight stays exactly zero under the fused Adan and Adam: zero gradient, zero moments, zero update.

On device tensors the event is three launches of csrc/prune.hip (ops.kth_abs, ops.prune_masks, ops.mask_mul) and one host read; on CPU
tensors it is a stock-torch restatement (torch.kthvalue, compare, multiply) that the tests use as the oracle of the kernels."""
import numpy as np
import torch

from . import _lib as L
from . import ops


def prunable(model):
    """[(name, parameter)] of the prunable set, in named_parameters() order."""
    return [(n, p) for n, p in model.named_parameters() if p.dim() > 1 and not n.startswith("encoder.")]


def schedule(S, steps):
    """[(epoch, s_j)] for --prune_sparsity S over the epochs --prune_steps: the geometric schedule of the NeRV family,
    s_j = 1 - (1 - S) ** ((j + 1) / m) at the j-th of the m events in epoch order; the last target is S itself."""
    S = float(S)
    if not 0.0 <= S < 1.0:
        raise ValueError(f"prune sparsity {S} outside [0, 1)")
    epochs = sorted(int(e) for e in steps)
    if len(set(epochs)) != len(epochs) or not epochs:
        raise ValueError(f"prune steps {list(steps)}: distinct epochs, at least one")
    m = len(epochs)
    return [(e, S if j == m - 1 else 1.0 - (1.0 - S) ** ((j + 1) / m)) for j, e in enumerate(epochs)]


class Pruner:
    """The masks of a model's prunable set and the events that move them.

        masks        {name: uint8 tensor of the parameter's shape}, allocated ONCE as all ones: a captured step keeps valid pointers
        prune_to(s)  one event -> {'k', 'pruned', 'n', 'tau'}
        sparsity()   pruned fraction of the prunable set, from the masks
        state_dict() / load_state_dict()   the masks bit-packed (numpy.packbits), their shapes and the index of the last event of the run

    optimizer: the run's optimizer.  Its per-element state tensors of the prunable parameters are masked at every event, and a fused
    optimizer of this package (optimizer.Adan / Adam) is told the masks (set_grad_masks) so engine.TrainStep can mask the gradients."""

    def __init__(self, model, optimizer=None):
        self.model, self.optimizer = model, optimizer
        self.named = prunable(model)
        if not self.named:
            raise ValueError("Pruner: the model has no prunable parameter")
        self.n = sum(p.numel() for _, p in self.named)
        self.masks = {n: torch.ones(p.shape, dtype=torch.uint8, device=p.device) for n, p in self.named}
        self.step_index = -1                                  # index (in the schedule) of the last event that ran
        self._table = None                                    # device: ops.PruneTable over (parameters, masks)
        self.on_device = all(p.is_cuda for _, p in self.named)
        if optimizer is not None and hasattr(optimizer, "set_grad_masks") and self.on_device:
            optimizer.set_grad_masks({p: self.masks[n] for n, p in self.named})

    # ---- the event ----------------------------------------------------------------------------------------------------
    def _state_tensors(self):
        """(state tensor, mask) of every per-element optimizer state of a prunable parameter (Adan: exp_avg, exp_avg_sq, exp_avg_diff,
        neg_pre_grad -- with an unmasked previous gradient g - g_prev would push a pruned weight off zero on the next step)."""
        pairs = []
        if self.optimizer is None:
            return pairs
        for n, p in self.named:
            for v in self.optimizer.state.get(p, {}).values():
                if torch.is_tensor(v) and v.shape == p.shape and v.dtype == p.dtype:
                    pairs.append((v, self.masks[n]))
        return pairs

    @torch.no_grad()
    def prune_to(self, s):
        """Prune to total sparsity s in [0, 1).  Raises ValueError for a NaN in the prunable set."""
        s = float(s)
        if not 0.0 <= s < 1.0:
            raise ValueError(f"prune_to: sparsity {s} outside [0, 1)")
        k = int(round(s * self.n))
        if k == 0:
            return {"k": 0, "pruned": self.pruned(), "n": self.n, "tau": 0.0}
        event = self._event_device if self.on_device else self._event_host
        pruned, tau, nan = event(k)
        if nan:
            raise ValueError("prune_to: a prunable parameter holds a NaN")
        return {"k": k, "pruned": pruned, "n": self.n, "tau": tau}

    def _event_device(self, k):
        params = [p.data for _, p in self.named]
        masks = [self.masks[n] for n, _ in self.named]
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise L.BnervError("Pruner: the HIP path needs contiguous fp32 parameters")
        key = tuple((p.data_ptr(), m.data_ptr(), p.numel()) for p, m in zip(params, masks))
        if self._table is None or self._table.key != key:
            self._table = ops.PruneTable(params, masks, "Pruner")
        out = self._table.kth_abs(k)
        self._table.prune_masks(out)                          # (out[0]: the bits of tau)
        pairs = self._state_tensors()
        if pairs:
            ops.mask_mul([v for v, _ in pairs], [m for _, m in pairs])
        host = out.cpu()                                      # the one host read of the event
        flags = int(host[1])
        if flags & (ops.KTH_FLAG_RANK | ops.KTH_FLAG_DESC):
            raise L.BnervError(f"Pruner: bnerv_kth_abs flagged its arguments (flags {flags})")
        return int(host[2:4].view(torch.int64)), float(host[0:1].view(torch.float32)), bool(flags & ops.KTH_FLAG_NAN)

    def _event_host(self, k):
        mags = torch.cat([p.detach().abs().reshape(-1) for _, p in self.named])
        if torch.isnan(mags).any():
            return 0, float("nan"), True
        tau = torch.kthvalue(mags, k).values
        pruned = 0
        for n, p in self.named:
            keep = p.detach().abs() > tau
            self.masks[n].copy_(keep)
            p.data.mul_(keep.to(p.dtype))
            pruned += int(keep.numel() - keep.sum())
        for v, m in self._state_tensors():
            v.mul_(m.to(v.dtype))
        return pruned, float(tau), False

    def _kept(self):
        return int(sum(int(m.sum()) for m in self.masks.values()))

    def pruned(self):
        """Number of pruned elements, from the masks (a host read)."""
        return self.n - self._kept()

    def sparsity(self):
        return self.pruned() / self.n

    # ---- checkpoint ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"masks": {n: torch.from_numpy(np.packbits(m.cpu().numpy().reshape(-1))) for n, m in self.masks.items()},
                "shapes": {n: tuple(m.shape) for n, m in self.masks.items()},
                "step_index": self.step_index}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Restores masks (into the tensors that exist: their addresses stay) and the event index; the weights come from the model's own
        checkpoint, where the pruned entries are zeros already."""
        if set(sd["masks"]) != set(self.masks):
            raise ValueError("Pruner.load_state_dict: the checkpoint's prunable set is not this model's")
        for n, m in self.masks.items():
            if tuple(sd["shapes"][n]) != tuple(m.shape):
                raise ValueError(f"Pruner.load_state_dict: {n} is {tuple(sd['shapes'][n])} in the checkpoint, {tuple(m.shape)} in the model")
            packed = sd["masks"][n]
            packed = packed.cpu().numpy() if torch.is_tensor(packed) else np.asarray(packed, dtype=np.uint8)
            bits = np.unpackbits(packed, count=m.numel()).reshape(tuple(m.shape))
            m.copy_(torch.from_numpy(bits).to(m.device))
        self.step_index = int(sd["step_index"])
