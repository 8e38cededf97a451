"""Record the kernel family / pair form of every distinct conv, weight-gradient and pair call of one training step of a shipped
configuration -> tests/conv_route_pins.json (tests/test_conv_route_cpu.py::test_families_of_the_shipped_layers).

Runs without a device.  The model runs on CPU tensors against a stand-in for the library (as tests/test_ops_plumbing_cpu.py) that
answers the host queries from the real library and launches nothing, so tensor contents are never computed; tensors report
`is_cuda` so that the model takes the paths it takes on the GPU (the ConvNeXt encoder's pointwise weight gradients among them).

The families written here come from the library that is loaded, so the file is a recording, not a yardstick: check the printed counts
against the kernel names of a kernel trace of the same step (profiles/conv_route.md has the table) before committing it.

    python tools/record_route_pins.py            (c1, c3, c4, hnerv: one child process each)
"""
import collections
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "conv_route_pins.json")
CONFIGS = ("c1", "c3", "c4", "hnerv")
# answered by the real library: they size buffers or grids and touch no device
HOST_QUERIES = ("bnerv_conv_partial_rows", "bnerv_conv_tiles", "bnerv_tanh_grad_blocks", "bnerv_adan_table_blocks", "bnerv_adam_table_blocks",
                "bnerv_cnx_mlp_plan", "bnerv_dwconv_wgrad_plan")


def int_fields(d):
    return {n: getattr(d, n) for n, t in d._fields_ if t is not C.c_void_p}


def null_pointers(d):
    return [n for n, t in d._fields_ if t is C.c_void_p and not getattr(d, n)]


def set_pointers(d):
    return {n: getattr(d, n) for n, t in d._fields_ if t is C.c_void_p and getattr(d, n)}


class Recorder:
    """Stands in for the ctypes library: records the three routed entry points, answers host queries, launches nothing."""

    def __init__(self, real, names):
        self.real, self.names, self.records = real, names, []

    def __getattr__(self, name):
        if not name.startswith("bnerv_"):
            raise AttributeError(name)

        def call(*args):
            if name in HOST_QUERIES or name.endswith("_ws_bytes"):
                return getattr(self.real, name)(*args)
            if name == "bnerv_last_error":
                return b""
            descs = [a._obj for a in args if isinstance(getattr(a, "_obj", None), C.Structure)]
            if name == "bnerv_conv_igemm":
                fam = self.real.bnerv_conv_family(C.byref(descs[0]), None)
                self.records.append(("conv", int_fields(descs[0]), null_pointers(descs[0]), self.names.CONV_FAM[fam]))
            elif name == "bnerv_conv_wgrad":
                fam = self.real.bnerv_conv_wgrad_family(C.byref(descs[0]), None)
                self.records.append(("wgrad", int_fields(descs[0]), null_pointers(descs[0]), self.names.WGRAD_FAM[fam]))
            elif name == "bnerv_conv_wgrad_pair":
                conv, wgrad = descs
                form = self.real.bnerv_conv_wgrad_pair_form(C.byref(conv), C.byref(wgrad), None)
                shared = sorted([cn, wn] for cn, cv in set_pointers(conv).items() for wn, wv in set_pointers(wgrad).items()
                                if cv == wv and cn != "ctx" and wn != "ctx")
                self.records.append(("pair", int_fields(conv), null_pointers(conv), int_fields(wgrad), null_pointers(wgrad), shared,
                                     "none" if form < 0 else self.names.PAIR_FORM[form]))
                return 0 if form >= 0 else 1           # "not a pair": the caller issues the two stand-alone calls, which are recorded
            return 0
        return call


class StreamContext:
    def __init__(self):
        self.handle, self.keep, self.dx_queued = C.c_void_p(0x7F0000000F00), [], False


def record(cfg):
    sys.path.insert(0, ROOT)
    sys.argv = [sys.argv[0]]                            # bench.py parses the command line when a model is built
    import torch
    import bench
    from boosting_nerv_amd import _lib as L

    lib, ctx = Recorder(L.load(), L), StreamContext()
    L.load = lambda optional=(): lib
    L.stream = lambda: None
    L.ctx = lambda create=True: ctx
    L.require_device = lambda t, name="tensor": t
    torch.Tensor.is_cuda = property(lambda self: True)

    idx = torch.tensor([3 / 7], dtype=torch.float64)
    if cfg == "hnerv":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import hnerv_ref
        from boosting_nerv_amd.model_hnerv import HNeRV
        torch.manual_seed(1)
        model, h, w = HNeRV(hnerv_ref.h1_args()), 720, 1280
    else:
        _, model = bench.build(cfg)
        h, w = bench.RECIPES[cfg]["h"], bench.RECIPES[cfg]["w"]
    if hasattr(model, "forward_encoder"):               # the models with a content encoder take the frame, the others its index
        out = model(torch.rand(1, 3, h, w), norm_idx=idx)
    else:
        out = model(idx, norm_idx=idx)
    img = out[0] if isinstance(out, (tuple, list)) else out
    torch.autograd.backward(img, torch.ones_like(img))

    print(cfg, type(model).__name__, "image", tuple(img.shape), len(lib.records), "calls")
    for key, n in sorted(collections.Counter((r[0], r[-1]) for r in lib.records).items()):
        print(f"    {key[0]:6s} {key[1]:12s} {n}")
    distinct = []
    for rec in json.loads(json.dumps(lib.records)):
        if rec not in distinct:
            distinct.append(rec)
    return distinct


def main():
    if len(sys.argv) > 1:                               # child: one configuration, its pins on the last line of the output
        print(json.dumps(record(sys.argv[1]), separators=(",", ":")))
        return
    pins = {}
    for cfg in CONFIGS:
        lines = subprocess.run([sys.executable, os.path.abspath(__file__), cfg], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
        print("\n".join(lines[:-1]))
        pins[cfg] = json.loads(lines[-1])
    with open(OUT, "w") as f:
        json.dump(pins, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
