"""The launches of the loss entry points, for comparing two builds of csrc/loss.hip under a kernel trace (profiles/loss_plumbing.md):
    rocprofv3 --kernel-trace -d DIR -- python tools/loss_launches.py [--lib PATH]     one eager pass over the calls below
    python tools/loss_launches.py --lines DIR                                         DIR's trace as `kernel grid wg lds` lines, in issue order (lds: every LDS column of the trace)
The calls, at (2, 3, 176, 208) (even pyramid) and (2, 3, 180, 270) (odd): L1, L1_freq, Fusion10, Fusion10_freq, Fusion6, L1_ssim_freq with a
gradient, a value-only Fusion10_freq, ops.msssim, ops.ssim, ops.psnr.  Equal lines = the same kernels on the same grids with the same LDS."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((2, 3, 176, 208), (2, 3, 180, 270))
TYPES = ("L1", "L1_freq", "Fusion10", "Fusion10_freq", "Fusion6", "L1_ssim_freq")


def lines(trace_dir):
    f = sorted(glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True))[-1]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"), "/".join(r[k] for k in r if "LDS" in k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--lines", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.lines:
        return lines(a.lines)
    if a.lib:
        os.environ["BNERV_LIB"] = os.path.abspath(a.lib)
    import torch
    from boosting_nerv_amd import ops
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        tgt = torch.rand(*shape, generator=g)
        pred = (tgt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1).to("cuda:0")
        tgt = tgt.to("cuda:0")
        for lt in TYPES:
            ops.loss_value_grad_stats(pred, tgt, lt)
        ops.loss_with_stats(pred, tgt, "Fusion10_freq")           # value only: `pred` does not require grad
        ops.msssim(pred, tgt); ops.ssim(pred, tgt); ops.psnr(pred, tgt)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
