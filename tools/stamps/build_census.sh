#!/bin/bash
# Wave-census build of the team kernels (-DPSDK_CENSUS, csrc/fused.hip) into tools/stamps/libpsdcascade_census.so: every
# wavefront of a fused launch records when and where it ran (tools/stamps/census.py reads the records).  The shipped library is
# never built this way.
#   CENSUS_EXTRA="-DPSDK_FAIR_FB=0"   more flags for fused.hip (the A/B switches of the kernel)
#   CENSUS_OUT=path.so             another output file (one per variant)
set -e
here=$(cd "$(dirname "$0")" && pwd)
csrc=$here/../../stabilizer-stream_amd/csrc
out=${CENSUS_OUT:-$here/libpsdcascade_census.so}
make -j4 -C "$csrc" >/dev/null
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
obj=$here/fused_census_$(basename "$out" .so).o
$HIPCC -x hip --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp \
    -Xclang -target-feature -Xclang -packed-fp32-ops -DPSDK_CENSUS ${CENSUS_EXTRA} \
    -I"$csrc" -c "$csrc/fused.hip" -o "$obj" 2> >(grep -v packed-fp32 >&2)
others=$(ls "$csrc"/*.o | grep -v '/fused\.o$')
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-z,defs -o "$out" "$obj" $others
echo built "$out"
