#!/bin/bash
# Development aid: ab/<name>.so = the whole library as it was at git revision <rev> (A/B of two states of the tree on ONE box:
# SMPLPP_HIP_LIB=$PWD/ab/<name>.so python ...).   usage: [IK_FLAGS="-DSMPLPP_EVAL_STAMPS"] tools/build_rev.sh <name> <rev>
# Every file is compiled with this tree's build flags (smplpp_amd/build.py).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"; name=$1; rev=$2
T=/tmp/rev_$name; rm -rf $T; mkdir -p $T/smplpp_amd/csrc $T/include "$ROOT/ab"
(cd "$ROOT" && git archive $rev smplpp_amd/csrc include | tar -x -C $T)
objs=""
for src in $T/smplpp_amd/csrc/*.hip; do
  b=$(basename $src); extra=""
  [ "$b" = ik.hip ] && extra="$IK_FLAGS"
  eval "$(python3 "$ROOT/smplpp_amd/build.py" --compile-cmd $src $T/$b.o $extra)" &
  objs="$objs $T/$b.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/ab/$name.so" $objs
echo "built ab/$name.so from $rev"
