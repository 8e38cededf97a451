"""TEST INFRASTRUCTURE (helper, not a test) -- the HNeRV baseline (reference model_hnerv.py:11-158, encoder form) and one
torch.optim.Adam step restated as plain functions over a state_dict, on stock torch ops in whatever dtype / device the state_dict has.
Pinned to golden vectors of the REAL reference by tests/test_hnerv_cpu.py; it is the float64 / stock-ops yardstick of the GPU tests and
of tools/khnerv.py."""
import hashlib
import math

import torch
import torch.nn.functional as F

from oracle import cpu_ref


def h1_args():
    """regression/bunny/hnerv.sh at --modelsize 1.525 (fc_dim 96 from the size solver)."""
    from oracle import configs
    return configs._base(model="HNeRV", embed="", enc_strds=[5, 2, 2, 2, 2], enc_dim="64_16", dec_strds=[5, 2, 2, 2, 2], dec_blks=[1, 1, 1, 1, 1],
                         ks="0_1_5", reduce=1.2, lower_width=12, fc_dim=96, conv_type=["convnext", "pshuffel"], act="gelu", sft_block="none")


def tiny_args():
    from oracle import configs
    return configs._base(model="HNeRV", enc_strds=[5, 2, 2], enc_dim="16_4", dec_strds=[5, 2, 2], dec_blks=[1, 1, 2], ks="0_1_5", reduce=1.2,
                         lower_width=6, fc_dim=10, conv_type=["convnext", "pshuffel"], act="gelu", sft_block="none", embed="")


def decoder_sha(sd):
    """SHA-256 over (key, fp32 bytes) of every non-encoder entry of a state_dict, in its order."""
    h = hashlib.sha256()
    for k, v in sd.items():
        if not k.startswith("encoder."):
            h.update(k.encode())
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _n_decoder(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("decoder."))


def decoder_forward(sd, img_embed, return_list=False):
    """decoder[0] (1x1 conv + GELU), the up-conv blocks (conv + PixelShuffle + GELU), 3x3 head + tanh * 0.5 + 0.5."""
    lst = [img_embed]
    x = F.gelu(F.conv2d(img_embed, sd["decoder.0.conv.downconv.weight"], sd["decoder.0.conv.downconv.bias"]))
    lst.append(x)
    n = _n_decoder(sd)
    for i in range(1, n):
        w, b = sd[f"decoder.{i}.conv.upconv.0.weight"], sd[f"decoder.{i}.conv.upconv.0.bias"]
        nxt = sd[f"decoder.{i + 1}.conv.upconv.0.weight"] if i + 1 < n else sd["head_layer.weight"]
        s = int(round(math.sqrt(w.shape[0] / nxt.shape[1])))
        x = F.conv2d(x, w, b, padding=(w.shape[-1] - 1) // 2)
        x = F.gelu(F.pixel_shuffle(x, s) if s > 1 else x)
        lst.append(x)
    img = cpu_ref.out_img(F.conv2d(x, sd["head_layer.weight"], sd["head_layer.bias"], padding=1))
    return (img, lst) if return_list else img


def forward(sd, frame, return_list=False):
    return decoder_forward(sd, cpu_ref.convnext_encoder(frame, sd, "encoder"), return_list)


def l2_loss(img, target):
    return F.mse_loss(img, target)


class AdamState:
    """torch.optim.Adam defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) over a list of tensors."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params, self.lr, self.betas, self.eps, self.t = params, lr, betas, eps, 0
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]

    @torch.no_grad()
    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            p.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-self.lr / bc1)


def train_step(sd, adam, frame):
    """One step on one frame [1, 3, H, W]: returns (loss, psnr [1], img); `sd` values are leaf tensors with requires_grad."""
    img = forward(sd, frame)
    loss = l2_loss(img, frame)
    grads = torch.autograd.grad(loss, adam.params)
    psnr = cpu_ref.psnr_fn_single(img.detach(), frame)
    adam.step(grads)
    return loss.detach(), psnr, img.detach()


def trajectory(sd0, frames, order, lr=1e-3, dtype=torch.float32, device="cpu"):
    sd = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in sd0.items()}
    adam = AdamState(list(sd.values()), lr=lr)
    frames = frames.to(device=device, dtype=dtype)
    losses, psnrs = [], []
    for fi in order:
        l, p, _ = train_step(sd, adam, frames[fi:fi + 1])
        losses.append(float(l))
        psnrs.append(float(p))
    return losses, psnrs, {k: v.detach() for k, v in sd.items()}
