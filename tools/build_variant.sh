#!/bin/bash
# Diagnostic / ablation build of the library: bash tools/build_variant.sh NAME -DFLAG [-DFLAG ...]  ->  stofnet_amd/libstof_NAME.so
# (only one source is rebuilt with the flags -- SRC=convstack (default) | gradpeak | hilbert | ...; the other objects are those of
# the last regular build, stofnet_amd/build/; use with STOF_LIB_PATH=stofnet_amd/libstof_NAME.so)
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p /tmp/stof_variant_$name
src=${SRC:-convstack}
extra=$(python -c "import sys; from stofnet_amd.build import EXTRA_FLAGS; print(' '.join(EXTRA_FLAGS.get(sys.argv[1] + '.hip', [])))" "$src")
objs=$(python -c "import sys; from stofnet_amd.build import SOURCES; print(' '.join('stofnet_amd/build/' + s.rsplit('.', 1)[0] + '.o' for s in SOURCES if s.rsplit('.', 1)[0] != sys.argv[1]))" "$src")
hipcc -O3 -std=c++17 -fPIC -fconstexpr-steps=100000000 --offload-arch=gfx950 -x hip $extra "$@" -c stofnet_amd/csrc/$src.hip -o /tmp/stof_variant_$name/$src.o
hipcc -shared -fPIC --offload-arch=gfx950 -o stofnet_amd/libstof_$name.so /tmp/stof_variant_$name/$src.o $objs
echo stofnet_amd/libstof_$name.so
