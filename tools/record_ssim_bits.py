"""Record the bits of the SSIM / MS-SSIM losses at the small shapes of tests/test_gpu_ssim_filter.py.

Run ONCE on the GPU with the library whose results are to be kept (the commit BEFORE a change of the filter bodies):
    python tools/record_ssim_bits.py [out.npz]          (default tests/golden/ssim_filter_bits.npz)
    python tools/record_ssim_bits.py --check FILE       (run again and compare with FILE: is the operator reproducible here?)

The fixture holds the inputs by SEED only (plus a SHA-256 of their bytes, so that a test notices a generator that drifted) and the
outputs as raw float32: loss, per-sample stats and the gradient of every case.  One case's gradient (2 x 3 x 180 x 270 = 1.17 MB) is
larger than the whole fixture may be: of that case the file keeps the LAST plane raw and the SHA-256 of the whole gradient's bytes --
equal digests are equal bits, which is what the test asks of every case.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name, loss type, shape, seed, elements past a 16-byte boundary (0 = as allocated), what the gradient is kept as
CASES = [
    ("ms_even_wide", "Fusion10_freq", (1, 1, 176, 224), 101, 0, "full"),     # even pyramid, W % 4 == 0: wide path, full and partial tiles
    ("ms_odd_scalar", "Fusion10", (1, 1, 163, 171), 102, 0, "full"),         # odd sides from level 0: scalar path, padded pools
    ("ms_odd_deeper", "Fusion10_freq", (2, 3, 180, 270), 103, 0, "digest"),  # odd deeper levels, W % 4 != 0, B * C > 1
    ("ms_unaligned", "Fusion10", (1, 1, 192, 352), 104, 1, "full"),          # W % 4 == 0 but a base 4 bytes past the boundary: scalar fallback
    ("ss_one_tile", "SSIM", (1, 3, 17, 45), 105, 0, "full"),                 # one partial tile, valid region smaller than a tile
    ("ss_two_tiles", "SSIM", (2, 1, 33, 70), 106, 0, "full"),
    ("ss_freq", "L1_ssim_freq", (1, 3, 48, 96), 107, 0, "full"),
]


def make_inputs(shape, seed):
    """(pred, target) on the CPU from the seed alone."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand(*shape, generator=g)
    pred = (tgt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return pred, tgt


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def place(t, shift, dev):
    """The tensor on the device, contiguous, `shift` floats past a 16-byte boundary."""
    if not shift:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * shift
    return v


def run_case(ops, case, dev):
    _, lt, shape, seed, shift, _ = case
    pred, tgt = make_inputs(shape, seed)
    loss, stats, grad = ops.loss_value_grad_stats(place(pred, shift, dev), place(tgt, shift, dev), lt)
    torch.cuda.synchronize()
    return loss.reshape(1).cpu().numpy(), stats.cpu().numpy(), grad.cpu().numpy()


def record(dev):
    from boosting_nerv_amd import ops
    out, meta = {}, []
    for case in CASES:
        name, lt, shape, seed, shift, keep = case
        pred, tgt = make_inputs(shape, seed)
        loss, stats, grad = run_case(ops, case, dev)
        out[name + ".loss"] = loss
        out[name + ".stats"] = stats
        out[name + ".grad"] = grad if keep == "full" else grad[-1, -1]
        meta.append({"name": name, "loss_type": lt, "shape": list(shape), "seed": seed, "shift": shift, "keep": keep,
                     "inputs_sha256": digest(pred.numpy(), tgt.numpy()), "grad_sha256": digest(grad)})
    out["cases"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return out


def main():
    dev = torch.device("cuda:0")
    args = sys.argv[1:]
    if args and args[0] == "--check":
        old = np.load(args[1])
        new = record(dev)
        bad = [k for k in new if not (old[k].shape == new[k].shape and old[k].tobytes() == new[k].tobytes())]
        print("reproduced" if not bad else f"DIFFERS: {bad}")
        sys.exit(1 if bad else 0)
    path = args[0] if args else os.path.join(ROOT, "tests", "golden", "ssim_filter_bits.npz")
    out = record(dev)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
