"""Record a library build's answers to the three long-standing host queries of the conv entry points over the table of
tests/conv_route_table.py -> tests/conv_route_answers.json (the yardstick of tests/test_conv_route_cpu.py: recorded from the commit BEFORE
a change to the kernel selection, compared at the change).  No device is touched.

    BNERV_LIB=/path/to/parent/libbnerv_hip.so python tools/record_conv_route.py [out.json]
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv_route_table as T                                  # noqa: E402
from boosting_nerv_amd import _lib as L                       # noqa: E402


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def conv_answers(lib, r):
    """[partial rows, split-K workspace bytes] of a conv row."""
    d = T.conv_desc(r)
    return with_env(r["env"], lambda: [lib.bnerv_conv_partial_rows(C.byref(d)), lib.bnerv_conv_splitk_ws_bytes(C.byref(d))])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "conv_route_answers.json")
    lib = L.load(optional=("bnerv_conv_family", "bnerv_conv_wgrad_family", "bnerv_conv_wgrad_pair_form"))
    ans = {"conv": [conv_answers(lib, r) for r in T.conv_rows()],
           "conv_changed": [conv_answers(lib, r) for r in T.changed_rows()],
           "wgrad_ws_bytes": [lib.bnerv_conv_wgrad_ws_bytes(*d) for d in T.wgrad_dims()]}
    with open(out, "w") as f:
        json.dump(ans, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(ans['conv'])} conv rows, {len(ans['wgrad_ws_bytes'])} weight-gradient dimension tuples from {L.LIB_PATH}")


if __name__ == "__main__":
    main()
