#!/bin/bash
# Registers / scratch / occupancy / LDS of the team kernels as the compiler reports them (no GPU needed), with the flags the
# Makefile uses for their files: the packet kernel (team_kernel) and the four kernels on team_walk.h -- team_walk_kernel,
# and tie_fix_kernel of trueknn_tail.hip, bigk_walk_kernel of trueknn_bigk.hip, query_walk_kernel of trueknn_query.hip.
#   scripts/team_resources.sh [extra -D flags]
cd "$(dirname "$0")/../owlraytracing_amd/csrc"
for src in trueknn_team.hip trueknn_tail.hip trueknn_bigk.hip trueknn_query.hip; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -fno-slp-vectorize \
    -I../../include -I../../include/owl_shims -I. -Wno-unused-result -Wno-bitwise-instead-of-logical "$@" \
    -Rpass-analysis=kernel-resource-usage -c $src -o /dev/null 2>&1 \
    | grep -A12 "Function Name:" | grep "Function Name\|  VGPRs:\|ScratchSize\|Occupancy\|LDS Size" | sed 's/.*remark: //; s/\[-Rpass.*//' | paste - - - - - \
    | sed 's/Function Name: //' | c++filt | grep "team_kernel\|team_walk_kernel\|tie_fix_kernel\|bigk_walk_kernel\|query_walk_kernel" \
    | sed 's/owlmi::(anonymous namespace):://g; s/owlmi:://g; s/([A-Za-z]*Args[^)]*)//; s/(std::conditional<[^)]*Args>::type)//' | tr -s ' \t' ' ' | cut -c1-160
done
