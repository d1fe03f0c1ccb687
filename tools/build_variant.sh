#!/bin/bash
# tools/build_variant.sh <tag> <extra hipcc -D flags...>  ->  ultrazoom_amd/libmewzoom_hip_<tag>.so
# e.g.  tools/build_variant.sh diag -DMZ_DIAG     (in-kernel cycle stamps of conv3r_kernel / conv3t_kernel: mz_diag.h, tools/stamp_probe_*.py)
set -euo pipefail
tag=$1; shift
here="$(cd "$(dirname "$0")/../ultrazoom_amd/csrc" && pwd)"
mkdir -p "$here/build"
source "$here/units.sh"
pids=()
for u in "${kernel_units[@]}"; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c "$here/$u.hip" -o "$here/build/${u}_$tag.o" &
    pids+=($!)
done
# the -D flags reach the host units too: they read the kernels' LDS geometry (mz_geo.h: MZ_GEMM1_S)
for u in "${host_units[@]}"; do
    /opt/rocm/bin/hipcc -O2 -std=c++17 -fPIC "$@" -c "$here/$u.cpp" -o "$here/build/${u}_$tag.o" &
    pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
objs=()
for u in "${kernel_units[@]}" "${host_units[@]}"; do objs+=("$here/build/${u}_$tag.o"); done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "$here/../libmewzoom_hip_$tag.so"
echo "built $tag"
