#!/bin/bash
# Experimental build of the library with extra -D flags (kernel A/B experiments on one GPU box):
#   tools/build_variant.sh NAME -DEXP_EX=1      ->  build/libNAME.so, selected at run time with BDDMMA_LIB=build/libNAME.so
# The sweep-bearing translation units (the Makefile's solver_*.o except solver_base.o) are rebuilt with the flags; the other objects of its OBJS
# are taken from the in-tree build (run make first).
set -e
name=$1; shift
cd "$(dirname "$0")/../bdd_amd/csrc"
mkdir -p ../../build/$name
objs=$(sed -n 's/^OBJS *= *//p' Makefile)
units=""; rest=""
for o in $objs; do
  u=${o%.o}
  case $u in
    solver_base|lbfgs) rest="$rest $o" ;;
    solver_*) units="$units $u" ;;
    *) rest="$rest $o" ;;
  esac
done
for u in $units; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -munsafe-fp-atomics -mllvm -amdgpu-kernarg-preload-count=16 -O3 -std=c++17 -fPIC -Wno-unused-function "$@" -c $u.hip -o ../../build/$name/$u.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build/lib$name.so $rest $(for u in $units; do echo ../../build/$name/$u.o; done)
echo built build/lib$name.so
