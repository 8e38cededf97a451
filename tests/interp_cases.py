"""Shared cases of the interpolation tests (test_interp_cpu.py, test_gpu_interp.py): the plans the issue names, written out by hand."""
import numpy as np

_T = float(np.float32(1) / np.float32(3))
_TT = float(np.float32(2) / np.float32(3))

# (n_frames, split) -> (stored frames, one (ia, ib, w) per frame; ia and ib index the stored list)
PLANS = {
    (5, "1_1_2"): ([0, 2, 4], [(0, 0, 0.0), (0, 1, 0.5), (1, 1, 0.0), (1, 2, 0.5), (2, 2, 0.0)]),
    (5, "1_1_3"): ([0, 3], [(0, 0, 0.0), (0, 1, _T), (0, 1, _TT), (1, 1, 0.0), (1, 1, 0.0)]),
    (10, "6_8_10"): ([0, 1, 2, 3, 4, 5], [(k, k, 0.0) for k in range(6)] + [(5, 5, 0.0)] * 4),
    (1, "1_1_2"): ([0], [(0, 0, 0.0)]),
}


def rows(plan):
    """A plan as a list of (ia, ib, w) tuples of Python numbers (w: the fp32 value, widened)."""
    return [(int(a), int(b), float(w)) for a, b, w in plan.tolist()]
