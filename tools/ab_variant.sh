#!/bin/bash
# Builds dynfu_amd/build/libdynfu_amd_<tag>.so with one source (or `all`) recompiled under extra flags (compile-time A/B):
#   bash tools/ab_variant.sh s6t solve6_assemble.hip -DDFA_S6_TIMING      then      DFA_LIB_PATH=dynfu_amd/build/libdynfu_amd_s6t.so python ...
#     (solve6_assemble.hip for tools/ns_assemble_phases.py, solve6_pattern.hip for tools/ns_pattern_phases.py; `all` serves both)
#   bash tools/ab_variant.sh prof all -DDFA_PCG_PROFILE -DDFA_DEV_AB
# Sources and flags come from dynfu_amd/build.py (one owner).
set -e
tag=$1; src=$2; shift 2
R=$(cd $(dirname $0)/.. && pwd)
B=$R/dynfu_amd/build
CC="/opt/rocm/bin/hipcc $(cd $R && python3 -c 'from dynfu_amd import build as B; print(" ".join(B.FLAGS))')"
SRCS=$(cd $R && python3 -c 'from dynfu_amd import build as B; print(" ".join(B.SOURCES))')
objs=""
for f in $SRCS; do
  o=${f%.*}; x=""; if [[ $f == *.cpp ]]; then x="-x hip"; fi
  if [ "$src" == all ] || [ "$f" == "$src" ]; then
    $CC "$@" $x -c $R/dynfu_amd/csrc/$f -o $B/${o}_$tag.o &
    objs="$objs $B/${o}_$tag.o"
  else
    objs="$objs $B/$o.o"
  fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $B/libdynfu_amd_$tag.so
echo $B/libdynfu_amd_$tag.so
