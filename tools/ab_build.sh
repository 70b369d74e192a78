#!/bin/bash
# Builds an A/B variant of the library: tools/ab/lib_<name>.so = the in-tree objects with <src>.hip
# recompiled under extra flags.  Usage: tools/ab_build.sh <name> <src (e.g. orbba)> <flags...>
# With REV=<git revision>, <src>.hip and the headers it is split into (csrc/<src>_*.h, where that revision
# has any) are taken from that revision instead of the working tree: they land beside the fetched source,
# where its quoted includes find them before the in-tree ones.
# (runs on the CPU side; the .so travels to the GPU box with the tree).
set -e
cd "$(dirname "$0")/../orb_slam2_refactored_amd/csrc"
name=$1; src=$2; shift 2
make -s
mkdir -p _build/ab ../../tools/ab
extra=""
case $src in orbx|orbm) extra="-mllvm -amdgpu-mfma-vgpr-form";; esac
[ -n "$NO_VGPR_FORM" ] && extra=""   # MFMA results in AGPRs (the compiler's default form)
file=$src.hip
if [ -n "$REV" ]; then
  dir=_build/ab/${src}_$name.rev
  rm -rf $dir && mkdir -p $dir
  file=$dir/$src.hip
  git show "$REV:orb_slam2_refactored_amd/csrc/$src.hip" > $file
  for h in $(git ls-tree --name-only "$REV" ./ | grep "^${src}_.*\.h$" || true); do
    git show "$REV:orb_slam2_refactored_amd/csrc/$h" > $dir/$h
  done
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result \
    -I../../include -I. $extra "$@" -c $file -o _build/ab/${src}_$name.o
objs=""
for o in _build/*.o; do
  b=$(basename $o .o)
  if [ "$b" = "$src" ]; then objs="$objs _build/ab/${src}_$name.o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/ab/lib_$name.so $objs
echo "tools/ab/lib_$name.so"
