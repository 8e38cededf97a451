"""Shared by test_resize_cpu.py and test_gpu_resize.py: the geometry set of the resize tests and a directory of random PNG frames."""
import os

import numpy as np

# (H, W, h, w)
GEOMETRIES = [(7, 5, 3, 2),           # truncated borders
              (16, 24, 8, 12),        # exact 2x, 8 taps
              (18, 33, 12, 22),       # 1.5x
              (12, 20, 24, 40),       # up-sampling: overshoot below 0 and above 1 before the clamp
              (9, 16, 9, 16),         # identity
              (36, 64, 17, 31),       # 9 taps, odd widths
              (11, 13, 29, 7),        # up on one axis, down on the other
              (64, 64, 1, 1),         # 64 taps, the limit
              (5, 7, 6, 9)]
IDS = [f"{H}x{W}-{h}x{w}" for H, W, h, w in GEOMETRIES]


def png_dir(path, n, H, W):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(11)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(os.path.join(path, f"f{i:03d}.png"))
    return str(path)
