#!/bin/bash
# Build this tree's libnumamma_gpu.so a second time, as build_ab/lib_NAME.so,
# for an A/B against another build (tools/ab_lib.sh):
#   tools/ab_build.sh NAME ["extra compiler flags"]
# The kernels carry no build-time variants: the other side of an A/B is
# another checkout (or an edited copy) of numamma_amd/ built the same way.
# Needs build/nmg_report.o and build/nmg_replay.o of a finished `make`.
set -e
cd "$(dirname "$0")/../numamma_amd"
NAME=$1; DEFS=$2
mkdir -p ../build_ab/obj_$NAME
for f in nmg_kernels nmg_route nmg_engine nmg_table nmg_submit nmg_route_host nmg_results nmg_multi nmg_placement; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../include -Icsrc -Wall -Wno-unused-result $DEFS \
    -x hip -c csrc/$f.hip -o ../build_ab/obj_$NAME/$f.o &
done
wait
for f in nmg_kernels nmg_route nmg_engine nmg_table nmg_submit nmg_route_host nmg_results nmg_multi nmg_placement; do [ -f ../build_ab/obj_$NAME/$f.o ] || { echo "compile of $f failed"; exit 1; }; done
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o ../build_ab/lib_$NAME.so ../build_ab/obj_$NAME/*.o build/nmg_report.o \
  build/nmg_replay.o -L/opt/rocm/lib -lrocprofiler-sdk-roctx
rm -rf ../build_ab/obj_$NAME
echo built build_ab/lib_$NAME.so
