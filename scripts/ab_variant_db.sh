#!/bin/bash
# Developer helper: one of the working tree's RT-DBSCAN files (SRC, default dbscan_union.hip: the group-union kernel and its
# build macros) with extra compile flags as owlraytracing_amd/libowl_mi355x_<tag>.so
#   scripts/ab_variant_db.sh b4 -DTKNN_DB_BOXES=4
#   SRC=dbscan_label.hip scripts/ab_variant_db.sh l1 -DSOMETHING=1
set -e
tag=$1; shift
src=${SRC:-dbscan_union.hip}; base=$(basename "$src" .hip)
cd "$(dirname "$0")/../owlraytracing_amd/csrc"
make >/dev/null
mkdir -p diagobj/ab
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden \
  -I../../include -I../../include/owl_shims -I. -Wno-unused-result -Wno-bitwise-instead-of-logical -Wno-unused-variable "$@" \
  -c $src -o diagobj/ab/${base}_$tag.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $(ls *.o | grep -v "^$base.o\$") diagobj/ab/${base}_$tag.o -o ../libowl_mi355x_$tag.so
echo built ../libowl_mi355x_$tag.so
