"""Compare the device code of two builds per kernel symbol.

    python tools/asm_symbols_diff.py DIR_A DIR_B

Each directory holds one `<unit>.s` per translation unit from
`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S <unit>.hip`.  Function bodies and kernel descriptors are compared after
dropping comments and the per-function numbering of local labels (function order may move between builds).  Used for host-only refactors
of csrc/ (profiles/conv_route.md): the count that differs must be 0.
"""
import os
import re
import sys

LOCAL_LABELS = ((re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), ".Lfunc"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"))


def symbols(path):
    """(function name -> body text, kernel name -> descriptor lines) of one assembly file."""
    bodies, descriptors = {}, {}
    func = kernel = None
    with open(path) as f:
        for line in f:
            m = re.match(r"\t\.type\t(\S+),@function", line)
            if m:
                func, body = m.group(1), []
                continue
            if func is not None:
                if re.match(r"\.Lfunc_end\d+:", line):
                    bodies[func] = "\n".join(body)
                    func = None
                    continue
                text = re.sub(r"\s*;.*$", "", line.rstrip())
                for pattern, repl in LOCAL_LABELS:
                    text = pattern.sub(repl, text)
                body.append(text)
            m = re.match(r"\t\.amdhsa_kernel (\S+)", line)
            if m:
                kernel = m.group(1)
                descriptors[kernel] = []
            elif kernel:
                if ".end_amdhsa_kernel" in line:
                    kernel = None
                else:
                    descriptors[kernel].append(line.rstrip())
    return bodies, descriptors


def main():
    dir_a, dir_b = sys.argv[1:3]
    compared = bad = 0
    for name in sorted(os.listdir(dir_a)):
        a, kd_a = symbols(os.path.join(dir_a, name))
        b, kd_b = symbols(os.path.join(dir_b, name))
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sum(1 for k in a if k in b and (a[k] != b[k] or kd_a.get(k) != kd_b.get(k)))
        print(f"{name}: parent {len(a)} symbols, change {len(b)}, only-parent {len(only_a)}, only-change {len(only_b)}, differ {differ}")
        for k in only_a[:3] + only_b[:3]:
            print("   ", k[:150])
        compared += len(set(a) & set(b))
        bad += differ + len(only_a) + len(only_b)
    print("compared", compared, "differ/missing", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
