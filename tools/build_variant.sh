#!/bin/bash
# Build a variant of the product library with extra -D flags into gpurun_variants/lib_<name>.so (A/B with tools/ab_libs.py).
#   tools/build_variant.sh abl27 "-DFA_RP16_ABL=27 -DFA_RP16_GATES=0"
set -e
name=$1; extra=$2
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/flashattention_kernel_project_amd/csrc
out=$root/gpurun_variants; obj=$out/obj_$name
mkdir -p "$obj"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -fvisibility=hidden -Wall -Wno-unused-function"
# the translation units of the product library: the Makefile's own list, so that a unit added there is linked here too
SRCS=$(sed -n 's/^SRCS *:= *//p' "$src/Makefile")
[ -n "$SRCS" ] || { echo "no SRCS line in $src/Makefile" >&2; exit 1; }
pids=()
for s in $SRCS; do
  # The only switches left are the pipeline kernel's instruments (FA_RP16_ABL, FA_RP16_GATES, FA_RP16_STAMPS), and only the
  # fa_fwd_rp16_*.hip family files see them.  Rebuilt with the flags: the d = 64 full-width family (fa_fwd_rp16_d64.hip) by
  # default, every family with ALL=1, exactly one translation unit with ONLY=<file.hip>; the rest are reused from the product build.
  if [ -n "$ONLY" ]; then want=$([ "$s" = "$ONLY" ] && echo 1 || echo 0); else want=-1; fi
  if [ "$want" = 1 ] || [ ! -f "$src/${s%.hip}.o" ]; then
    /opt/rocm/bin/hipcc $FLAGS $extra -c "$src/$s" -o "$obj/${s%.hip}.o" &
    pids+=($!)
  elif [ "$want" = 0 ]; then
    cp "$src/${s%.hip}.o" "$obj/${s%.hip}.o"
  elif [ "$s" = "fa_fwd_rp16_d64.hip" ] || { [ -n "$ALL" ] && [[ "$s" == fa_fwd_rp16_* ]]; } || [ ! -f "$src/${s%.hip}.o" ]; then
    /opt/rocm/bin/hipcc $FLAGS $extra -c "$src/$s" -o "$obj/${s%.hip}.o" &
    pids+=($!)
  else
    cp "$src/${s%.hip}.o" "$obj/${s%.hip}.o"
  fi
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $obj/*.o -o "$out/lib_$name.so"
echo "built $out/lib_$name.so"
