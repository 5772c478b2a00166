#!/bin/bash
# Registers, scratch and occupancy of every kernel in one .hip file, as the compiler reports them (no GPU
# needed):  scripts/kernel_resources.sh owlraytracing_amd/csrc/trueknn_team.hip [filter]
# (the packet kernel; the hand-over walk and the tie pass: trueknn_tail.hip, the k > 64 walk: trueknn_bigk.hip)
# (RT-DBSCAN's kernels by pass: dbscan_core.hip, dbscan_union.hip, dbscan_label.hip)
# and, with ISA=1, the gfx950 assembly in /tmp/<name>.s (look for v_cmp_*_i32 + s_and_saveexec in loops:
# wave-uniform values kept in VGPRs).
# EXTRA is passed on to hipcc: the Makefile builds some objects with flags of their own, and without them the numbers here are
# not the build's.  radius_knn.hip, knn_seed.hip, periodic_knn.hip and batch_knn.hip (and the other team kernels' files):
#   EXTRA=-fno-slp-vectorize scripts/kernel_resources.sh owlraytracing_amd/csrc/radius_knn.hip
# likewise radius_query.hip, radius_reduce.hip and local_pca.hip, whose walk and lane kernels are radius_walk.h's
# rad_walk_kernel<Rule> and rad_lane_kernel<Rule> (filter: rad_).
set -e
src=$1; filt=${2:-.}
dir=$(cd "$(dirname "$src")" && pwd); root=$(cd "$(dirname "$0")/.." && pwd)
flags="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -I$root/include -I$root/include/owl_shims -I$dir -Wno-unused-result -Wno-bitwise-instead-of-logical ${EXTRA:-}"
/opt/rocm/bin/hipcc $flags -Rpass-analysis=kernel-resource-usage -c "$src" -o /dev/null 2>&1 \
  | grep -A12 "Function Name:" | grep "Function Name\|SGPRs:\|VGPRs:\|ScratchSize\|Occupancy\|LDS Size" \
  | sed 's/.*remark: //; s/\[-Rpass.*//' | paste - - - - - - | grep "$filt" | sed 's/Function Name: //' | c++filt | sed 's/owlmi::(anonymous namespace):://g' | cut -c1-230
if [ "${ISA:-0}" = 1 ]; then
  out=/tmp/$(basename "$src" .hip).s
  /opt/rocm/bin/hipcc $flags -S --cuda-device-only -o "$out" "$src" 2>/dev/null
  echo "ISA in $out"
fi
