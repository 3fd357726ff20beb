#!/bin/bash
# A/B builds of the window kernels: tools/build_variants.sh name "-DFLAG=.. -DFLAG2=.." [name flags]...
# -> build_ab/libprcg_<name>.so (select one with PRCG_LIB=...; build_ab/ travels to the GPU box, not into git)
# The link line is the Makefile's object list (make print-objs) with the one rebuilt object replaced.
set -e
mkdir -p build_ab
make -s
objs=$(make -s print-objs)
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude $flags -c new_cg_variants_amd/csrc/prcg_win.hip -o build_ab/win_$name.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_ab/libprcg_$name.so ${objs/new_cg_variants_amd\/csrc\/prcg_win.o/build_ab\/win_$name.o} -ldl
  echo built build_ab/libprcg_$name.so
done
