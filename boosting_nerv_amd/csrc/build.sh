#!/usr/bin/env bash
# Build libbnerv_hip.so (gfx950 only) in-tree.  Usage: build.sh [-j N]
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libbnerv_hip.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
mkdir -p _obj
pids=()
UNITS="abi conv conv4 conv5 convs convbf wgrad wgrad1 eltwise head3 stem gemm dense optim loss dwconv cem lnorm codec yuv huff rans ransenc ransw ranst prune huffz hufft interp resize upyuv upyuvloss"
for f in $UNITS; do
  stale=0
  for h in *.h ../../include/bnerv.h; do [ $h -nt _obj/$f.o ] && stale=1; done
  if [ ! -f _obj/$f.o ] || [ $f.hip -nt _obj/$f.o ] || [ $stale = 1 ]; then
    $HIPCC $FLAGS -c $f.hip -o _obj/$f.o &
    pids+=($!)
  fi
done
if [ ! -f _obj/ans.o ] || [ ans.cpp -nt _obj/ans.o ] || [ common.h -nt _obj/ans.o ] || [ ../../include/bnerv.h -nt _obj/ans.o ]; then
  $HIPCC -x hip $FLAGS -c ans.cpp -o _obj/ans.o &
  pids+=($!)
fi
if [ ! -f _obj/huffh.o ] || [ huff.cpp -nt _obj/huffh.o ] || [ common.h -nt _obj/huffh.o ] || [ huff_code.h -nt _obj/huffh.o ] || [ ../../include/bnerv.h -nt _obj/huffh.o ]; then
  $HIPCC -x hip $FLAGS -c huff.cpp -o _obj/huffh.o &
  pids+=($!)
fi
if [ ! -f _obj/huffzh.o ] || [ huffz.cpp -nt _obj/huffzh.o ] || [ huff_code.h -nt _obj/huffzh.o ] || [ ../../include/bnerv.h -nt _obj/huffzh.o ]; then
  $HIPCC -x hip $FLAGS -c huffz.cpp -o _obj/huffzh.o &
  pids+=($!)
fi
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT $(printf '_obj/%s.o ' $UNITS) _obj/ans.o _obj/huffh.o _obj/huffzh.o
echo "built $(realpath $OUT)"
