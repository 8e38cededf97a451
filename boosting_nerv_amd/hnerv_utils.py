"""Host-side utilities -- mirror of the reference's hnerv_utils.py for the train path: dataset, split, LR schedule,
loss_fn / psnr / ms-ssim entry points (HIP kernels underneath), post-hoc 8-bit quantisation used by evaluate(), and the
distributed scalar reduction.  Same function names, argument meaning and return conventions as the reference; lines cited
per function."""
import math
import os
import random

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
from torch.utils.data import Dataset

from . import ops, synth


# ----------------------------------------------------------------------------------------------------------------------
# dataset                                                                               reference hnerv_utils.py:16-56
# ----------------------------------------------------------------------------------------------------------------------
def _to_tensor(pil_img):
    arr = np.asarray(pil_img, dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1))).to(torch.float32).div(255)    # == ToTensor()


def _center_crop(img, ch, cw):
    w, h = img.size
    top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
    return img.crop((left, top, left + cw, top + ch))


def frame_hw(args):
    """(H, W) of the frames a run trains on, decodes and stores: the --resize_list size when one is given, the --crop_list size otherwise."""
    from .resize import parse_resize
    size = parse_resize(getattr(args, "resize_list", "-1"))
    return size if size is not None else tuple(int(x) for x in args.crop_list.split("_")[:2])


class VideoDataSet(Dataset):
    """Sorted directory of frames (PNG/JPG), centre-cropped to --crop_list, ToTensor, norm_idx = (idx+1)/N  (:19-47).
    ``--resize_list H_W`` resamples every cropped frame to H x W with the antialiased bicubic of resize.py: crop, then
    resize, for every kind of source -- resize.resize_reference here, ops.resize_bicubic (the same bits) when the clip is made resident.
    ``--data_path synthetic:bunny | synthetic:uvg | synthetic:NxHxW`` selects the in-repo deterministic generator instead
    (no dataset ships with the reference).  A ``--data_path`` ending in ``.yuv`` is a raw planar YUV 4:2:0 clip (yuvio.YuvFile; --yuv_size,
    --yuv_fmt, --yuv_matrix, --yuv_range): same samples, same crop, decoded by the float64 restatement here and by the conversion kernel
    when the clip is made resident (to_device)."""

    def __init__(self, args):
        self.crop_h, self.crop_w = [int(x) for x in args.crop_list.split("_")[:2]]
        from .resize import axis_table, parse_resize
        self.frame_h, self.frame_w = frame_hw(args)
        self.resize = parse_resize(getattr(args, "resize_list", "-1"))          # None: the frames stay at the crop size
        if self.resize is not None:
            axis_table(self.crop_h, self.frame_h), axis_table(self.crop_w, self.frame_w)      # (ValueError over the tap limit, before any frame is read)
        self.synthetic = None
        self.yuv = None
        if str(args.data_path).lower().endswith(".yuv"):
            from . import yuvio
            w, h = yuvio.parse_size(args.yuv_size) if getattr(args, "yuv_size", None) else (None, None)
            self.yuv = yuvio.YuvFile(args.data_path, w, h, getattr(args, "yuv_fmt", None))
            self.yuv_matrix, self.yuv_range = getattr(args, "yuv_matrix", "bt709"), getattr(args, "yuv_range", "limited")
            self.yuv.crop_window((self.crop_h, self.crop_w))              # (raises for a clip smaller than --crop_list)
            self.samples = list(range(len(self.yuv)))
        elif str(args.data_path).startswith("synthetic:"):
            n, h, w = synth.parse_spec(args.data_path)
            if (h, w) != (self.crop_h, self.crop_w):
                h, w = self.crop_h, self.crop_w
            self.synthetic = synth.SyntheticVideo(n, h, w)
            self.samples = list(range(n))
            self._cache = {}
        else:
            self.samples = [os.path.join(args.data_path, x) for x in sorted(os.listdir(args.data_path))]
        if getattr(args, "interpolation", False) and len(self.samples) % 2 == 0:
            self.samples.pop()
        self.crop = True
        self.final_size = self.frame_h * self.frame_w
        self.embed_inter = getattr(args, "embed_inter", False) and getattr(args, "interpolation", False)
        if self.synthetic is None and self.yuv is None:
            from PIL import Image
            first = Image.open(self.samples[0]).convert("RGB")
            if not (first.height >= self.crop_h and first.width >= self.crop_w):
                raise NotImplementedError("frames smaller than --crop_list (bicubic up-sampling branch, hnerv_utils.py:29-31) are not supported")

    def __len__(self):
        return len(self.samples)

    def _load_crop(self, idx):
        """Frame idx at the crop size, before any resize."""
        if self.synthetic is not None:
            return self.synthetic.frame(idx)
        if self.yuv is not None:
            return torch.from_numpy(self.yuv.frame_rgb(self.samples[idx], (self.crop_h, self.crop_w), self.yuv_matrix, self.yuv_range))
        from PIL import Image
        return _to_tensor(_center_crop(Image.open(self.samples[idx]).convert("RGB"), self.crop_h, self.crop_w))

    def _load(self, idx):
        if self.synthetic is not None and idx in self._cache:
            return self._cache[idx]
        img = self._load_crop(idx)
        if self.resize is not None:
            from .resize import resize_reference
            img = resize_reference(img, self.resize)
        if self.synthetic is not None:
            self._cache[idx] = img
        return img

    def to_device(self, device, chunk=32):
        """The clip as a resident [N, 3, H, W] fp32 device tensor: a raw YUV clip goes up as it lies in the file and is converted there
        (YuvFile.to_device, no host fp32 frames); every other source is stacked on the host and uploaded.  Under --resize_list the frames go
        up at the crop size `chunk` at a time and are resampled into their slice of the clip (ops.resize_bicubic): the full-size clip never
        exists on the device."""
        if self.yuv is not None:
            return self.yuv.to_device(device, chunk=chunk, crop=(self.crop_h, self.crop_w), matrix=self.yuv_matrix, range=self.yuv_range,
                                      count=len(self.samples), resize=self.resize)
        if self.resize is None:
            return torch.stack([self[i]['img'] for i in range(len(self))]).to(device)
        device = torch.device(device)
        n = len(self)
        chunk = max(1, min(int(chunk), n))
        clip = torch.empty(n, 3, self.frame_h, self.frame_w, dtype=torch.float32, device=device)
        scratch = torch.empty(chunk * 3 * self.crop_h * self.frame_w, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            for i0 in range(0, n, chunk):
                i1 = min(i0 + chunk, n)
                full = torch.stack([self._load_crop(i) for i in range(i0, i1)]).to(device)
                ops.resize_bicubic(full, self.resize, out=clip[i0:i1], scratch=scratch)
            torch.cuda.current_stream().synchronize()
        return clip

    def __getitem__(self, idx):
        img = self._load(idx)
        norm_idx = float(idx + 1) / len(self.samples)
        if self.embed_inter:
            if idx % 2 == 0:
                pre_img, post_img = img, img
            else:
                pre_img, post_img = self._load(idx - 1), self._load(idx + 1)
            return {"img": img, "idx": idx, "norm_idx": norm_idx, "pre_img": pre_img, "post_img": post_img}
        return {"img": img, "idx": idx, "norm_idx": norm_idx}


class TransformInput(nn.Module):                                                         # reference hnerv_utils.py:59-84
    def __init__(self, args):
        super().__init__()
        self.inpanting = args.inpanting
        if "inpanting_fixed" in self.inpanting:
            self.inpaint_size = int(self.inpanting.split("_")[-1]) // 2

    @property
    def identity(self):
        """True when input == gt and the mask is all ones: the train loop then skips the two full-frame multiplies by one
        (train_nerv_all.py:343) -- identical result, 3 fewer passes over a frame."""
        return "inpanting" not in self.inpanting

    def forward(self, img, idx):
        if self.identity:
            return img, img, None
        gt = img.clone()
        h, w = img.shape[-2:]
        inpaint_mask = torch.ones((h, w), device=img.device)
        if "center" in self.inpanting:
            ih, iw = h // 8, w // 8
            cx, cy = int(0.5 * h), int(0.5 * w)
            inpaint_mask[cx - ih: cx + ih, cy - iw: cy + iw] = 0
        elif "fixed" in self.inpanting:
            for cx, cy in [(1 / 2, 1 / 2), (1 / 4, 1 / 4), (1 / 4, 3 / 4), (3 / 4, 1 / 4), (3 / 4, 3 / 4)]:
                cx, cy = int(cx * h), int(cy * w)
                inpaint_mask[cx - self.inpaint_size: cx + self.inpaint_size, cy - self.inpaint_size: cy + self.inpaint_size] = 0
        inp = (img * inpaint_mask).clamp(min=0, max=1)
        return inp, gt, inpaint_mask.detach()


def data_split(img_list, split_num_list, shuffle_data, rand_num=0):
    """Periodic train / validation partition of the frame list (--data_split a_b_c, reference hnerv_utils.py:87-98): inside every
    period of c frames the first a are training frames and those from position b on are held out.  `shuffle_data` permutes the
    list first with Random(rand_num) -- the same generator call as the reference, so the same split."""
    n_seen, n_train_end, period = split_num_list
    frames = list(img_list)
    if shuffle_data:
        random.Random(rand_num).shuffle(frames)
    train = [f for pos, f in enumerate(frames) if pos % period < n_seen]
    held_out = [f for pos, f in enumerate(frames) if pos % period >= n_train_end]
    return train, held_out


# ----------------------------------------------------------------------------------------------------------------------
# interpolation from stored embeddings: which frames a file stores, and how every other frame's embedding follows
# from theirs.  Host only; csrc/interp.hip (ops.embed_expand) executes the plan
# ----------------------------------------------------------------------------------------------------------------------
INTERP_ENTRY = np.dtype([("ia", "<i4"), ("ib", "<i4"), ("w", "<f4")])      # bnerv_interp_entry: one row of a plan, three dwords


def parse_split(split):
    """--data_split 'a_b_c' (or its three integers) -> [a, b, c]."""
    nums = [int(x) for x in split.split("_")] if isinstance(split, str) else [int(x) for x in split]
    if len(nums) != 3 or nums[2] < 1 or min(nums) < 0:
        raise ValueError(f"interp_plan: --data_split {split!r} is not a_b_c with c >= 1")
    return nums


def interp_plan(n_frames, split, shuffle_data=False):
    """(stored, plan) of an --interpolation --embed_inter_stored run over n_frames frames.
    stored: the training frames of data_split(range(N), split, False), ascending -- positions < a of every period of c frames.
    plan: [N] rows (ia, ib, w) of INTERP_ENTRY, ia and ib indices into `stored`, w fp32.  Stored frame stored[k]: (k, k, 0).  Every other
    frame t is derived -- held out or not: between its nearest stored frames stored[ia] < t < stored[ib] with
    w = fp32(t - stored[ia]) / fp32(stored[ib] - stored[ia]); with a stored frame on one side only, (k, k, 0) of that side.  With 1_1_2
    and an odd frame count this is the reference's rule: neighbours idx - 1 and idx + 1, w = 0.5.
    ValueError: no stored frame; shuffle_data (a shuffled split has no neighbours in time)."""
    if shuffle_data:
        raise ValueError("interp_plan: --shuffle_data permutes the frames before the split: a held-out frame has no neighbours in time to derive it from")
    n_frames = int(n_frames)
    stored, _ = data_split(list(range(n_frames)), parse_split(split), False)
    if not stored:
        raise ValueError(f"interp_plan: --data_split {split!r} over {n_frames} frames stores no frame")
    plan = np.zeros(n_frames, dtype=INTERP_ENTRY)
    k = 0                                                  # stored[k] is the nearest stored frame at or below t, once there is one
    for t in range(n_frames):
        while k + 1 < len(stored) and stored[k + 1] <= t:
            k += 1
        if stored[k] >= t or k + 1 == len(stored):         # stored itself, in front of the first stored frame, or behind the last
            plan[t] = (k, k, 0.0)
        else:
            plan[t] = (k, k + 1, np.float32(t - stored[k]) / np.float32(stored[k + 1] - stored[k]))
    return stored, plan


def check_interp_plan(plan, n_stored):
    """The plan as a contiguous INTERP_ENTRY array; ValueError for an index outside 0..n_stored-1 or a weight outside [0, 1) -- what whoever
    launches ops.embed_expand calls before the plan goes to the device."""
    plan = np.ascontiguousarray(plan, dtype=INTERP_ENTRY).reshape(-1)
    if plan.size == 0:
        raise ValueError("interp plan: no rows")
    for name in ("ia", "ib"):
        if int(plan[name].min()) < 0 or int(plan[name].max()) >= int(n_stored):
            raise ValueError(f"interp plan: {name} outside 0..{int(n_stored) - 1}")
    if not bool(np.all((plan["w"] >= 0) & (plan["w"] < 1))):
        raise ValueError("interp plan: a weight outside [0, 1)")
    return plan


def embed_expand_reference(src, plan):
    """numpy fp32 restatement of ops.embed_expand (csrc/interp.hip), bit for bit: src [S, P] -> [N, P].  ia == ib: copy; w == 0.5:
    0.5 * (L + R); otherwise (1 - w) * L + w * R with every operation rounded to fp32 on its own."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    plan = check_interp_plan(plan, src.shape[0])
    out = np.empty((plan.size,) + src.shape[1:], dtype=np.float32)
    half = np.float32(0.5)
    for t, (ia, ib, w) in enumerate(plan.tolist()):
        w = np.float32(w)
        if ia == ib:
            out[t] = src[ia]
        elif w == half:
            out[t] = half * (src[ia] + src[ib])
        else:
            out[t] = (np.float32(1.0) - w) * src[ia] + w * src[ib]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# post-hoc 8-bit quantisation used by evaluate() / quant_model (reference hnerv_utils.py:101-134, :183-186): eval-time
# reporting on stock torch ops, not part of the train hot path
# ----------------------------------------------------------------------------------------------------------------------
def quant_tensor(t, bits=8):
    """Uniform `bits`-bit quantisation of a tensor on the best of several affine grids: one (min, step) pair for the whole tensor
    (kept in fp32), and one pair per slice along every axis whose pair count stays below 2 % of the element count (stored as
    fp16, as they are what gets transmitted).  The grid with the smallest mean absolute reconstruction error wins (first one on
    ties).  Returns ({'quant': uint8 codes, 'min', 'scale'}, reconstructed tensor)."""
    top = 2 ** bits - 1
    grids = [(t.min(), (t.max() - t.min()) / top)]
    for axis in range(t.dim()):
        lo, hi = t.amin(axis, keepdim=True), t.amax(axis, keepdim=True)
        if lo.nelement() / t.nelement() < 0.02:
            grids.append((lo.to(torch.float16), ((hi - lo) / top).to(torch.float16)))
    best = None
    for lo, step in grids:
        lo_e, step_e = lo.expand_as(t), step.expand_as(t)
        codes = ((t - lo_e) / step_e).round().clamp(0, top)
        rebuilt = lo_e + step_e * codes
        err = (t - rebuilt).abs().mean()
        if best is None or err < best[0]:
            best = (err, codes, rebuilt, lo, step)
    _, codes, rebuilt, lo, step = best
    return {"quant": codes.to(torch.uint8), "min": lo, "scale": step}, rebuilt


def quant_tensor_sparse(t, bits=8):
    """quant_tensor for a pruned tensor: an element that is zero stays exactly +0.0 and takes no part in fitting the
    grids.  The candidate grids are quant_tensor's; `lo` and `hi` of a slice are taken over its kept (non-zero) elements only, a slice
    without one takes lo = 0, step = 0, and where step == 0 the codes are 0 and the rebuilt value is lo (nothing is divided by zero).
    The grid with the smallest sum of |t - rebuilt| over the kept elements wins (first one on ties).  Returns
    ({'quant', 'min', 'scale', 'keep'}, rebuilt) with keep = t != 0; on a tensor without zeros and without a constant slice every field
    equals quant_tensor's."""
    top = 2 ** bits - 1
    keep = t != 0
    big = torch.full_like(t, float("inf"))

    def fit(axis):
        lo = torch.where(keep, t, big).min() if axis is None else torch.where(keep, t, big).amin(axis, keepdim=True)
        hi = torch.where(keep, t, -big).max() if axis is None else torch.where(keep, t, -big).amax(axis, keepdim=True)
        empty = lo > hi                                    # no kept element in the slice: (+inf, -inf)
        lo, hi = torch.where(empty, torch.zeros_like(lo), lo), torch.where(empty, torch.zeros_like(hi), hi)
        return lo, (hi - lo) / top

    grids = [fit(None)]
    for axis in range(t.dim()):
        lo, step = fit(axis)
        if lo.nelement() / t.nelement() < 0.02:
            grids.append((lo.to(torch.float16), step.to(torch.float16)))
    best = None
    for lo, step in grids:
        lo_e, step_e = lo.expand_as(t), step.expand_as(t)
        flat = step_e == 0
        codes = ((t - lo_e) / torch.where(flat, torch.ones_like(step_e), step_e)).round().clamp(0, top)
        codes = torch.where(flat | ~keep, torch.zeros_like(codes), codes)
        rebuilt = torch.where(keep, lo_e + step_e * codes, torch.zeros_like(codes))
        err = ((t - rebuilt).abs() * keep).sum()
        if best is None or err < best[0]:
            best = (err, codes, rebuilt, lo, step)
    _, codes, rebuilt, lo, step = best
    return {"quant": codes.to(torch.uint8), "min": lo, "scale": step, "keep": keep}, rebuilt


def dequant_tensor(quant_t):
    q, tmin, scale = quant_t["quant"], quant_t["min"], quant_t["scale"]
    return tmin.expand_as(q) + scale.expand_as(q) * q


# ----------------------------------------------------------------------------------------------------------------------
# distributed helpers                                                               reference hnerv_utils.py:213-248
# ----------------------------------------------------------------------------------------------------------------------
def all_reduce(tensors, average=True):
    for tensor in tensors:
        dist.all_reduce(tensor, async_op=False)
    if average:
        world_size = dist.get_world_size()
        for tensor in tensors:
            tensor.mul_(1.0 / world_size)
    return tensors


def is_dist_avail_and_initialized():
    return dist.is_available() and dist.is_initialized()


def get_rank():
    return dist.get_rank() if is_dist_avail_and_initialized() else 0


def get_world_size():
    return dist.get_world_size() if is_dist_avail_and_initialized() else 1


def worker_init_fn(worker_id):
    worker_seed = torch.initial_seed() % 2 ** 32
    np.random.seed(worker_seed)
    random.seed(worker_seed)


def RoundTensor(x, num=2, group_str=False):                                           # reference hnerv_utils.py:277-289
    if group_str:
        return "/".join(",".join(str(round(ele, num)) for ele in x[i].tolist()) for i in range(x.size(0)))
    return ",".join(str(round(ele, num)) for ele in x.flatten().tolist())


# ----------------------------------------------------------------------------------------------------------------------
# LR schedule                                                                       reference hnerv_utils.py:292-322
# ----------------------------------------------------------------------------------------------------------------------
def adjust_lr(optimizer, cur_epoch, cur_iter, args):
    if "hybrid" in args.lr_type:
        up_ratio, up_pow, down_pow, min_lr, final_lr = [float(x) for x in args.lr_type.split("_")[1:]]
        if cur_epoch < up_ratio:
            lr_mult = min_lr + (1.0 - min_lr) * (cur_epoch / up_ratio) ** up_pow
        else:
            lr_mult = 1 - (1 - final_lr) * ((cur_epoch - up_ratio) / (1.0 - up_ratio)) ** down_pow
    elif "cosine" in args.lr_type:
        up_ratio, up_pow, min_lr = [float(x) for x in args.lr_type.split("_")[1:]]
        if cur_epoch < up_ratio:
            lr_mult = min_lr + (1.0 - min_lr) * (cur_epoch / up_ratio) ** up_pow
        else:
            lr_mult = 0.5 * (math.cos(math.pi * (cur_epoch - up_ratio) / (1 - up_ratio)) + 1.0)
    elif "enerv_sch" in args.lr_type:
        all_iter = args.epochs * args.full_data_length
        now_iter = cur_epoch * args.full_data_length + cur_iter
        if now_iter < all_iter * 0.2:
            lr_mult = 0.1 + 0.9 * now_iter / (all_iter * 0.2)
        else:
            lr_mult = 0.5 * (math.cos(math.pi * (now_iter - all_iter * 0.2) / (all_iter - all_iter * 0.2)) + 1.0)
    else:
        raise NotImplementedError
    for param_group in optimizer.param_groups:
        param_group["lr"] = args.lr * lr_mult
    return args.lr * lr_mult


# ----------------------------------------------------------------------------------------------------------------------
# loss and metrics                                                           reference hnerv_utils.py:335-419
# ----------------------------------------------------------------------------------------------------------------------
def loss_fn(pred, target, loss_type="L2", batch_average=True, mask=None):
    """Value + gradient come from one fused HIP call.  Every variant of the reference is built: L1, L2, L1_freq, Fusion7/8 and the
    MS-SSIM mixes Fusion10/11/12, Fusion10_freq (bnerv_loss_fwd_bwd; MS-SSIM needs min(H, W) > 160), and the single-scale SSIM mixes
    SSIM, Fusion1-6, Fusion9, L1_ssim_freq (bnerv_loss_ssim_fwd_bwd; min(H, W) >= 11 -- a smaller frame raises NotImplementedError,
    where the reference skips the filter along the short side).
    mask ([H, W], inpainting): loss_fn(pred * mask, target * mask, ...) of train_nerv_all.py:343, bit for bit, without the two full-frame
    products in the autograd graph."""
    loss, stats = ops.loss_with_stats(pred, target, loss_type, mask=mask)
    if batch_average:
        return loss
    # per-sample values (no gradient path): stats[:,0]
    return stats[:, 0]


def psnr_fn_device(output, gt):
    """Per-sample PSNR as a DEVICE tensor (no host sync) -- what the train loop accumulates."""
    return ops.psnr(output, gt)


def psnr_fn_single(output, gt):
    return psnr_fn_device(output, gt).cpu()


def psnr_fn_batch(output_list, gt):
    return torch.stack([psnr_fn_single(o.detach(), gt.detach()) for o in output_list], 0).cpu()


def msssim_fn_single(output, gt):
    return ops.msssim(output.float().detach(), gt.detach()).cpu()


def msssim_fn_batch(output_list, gt):
    return torch.stack([msssim_fn_single(o.detach(), gt.detach()) for o in output_list], 0).cpu()
