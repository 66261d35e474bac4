#!/bin/bash
# calibration build of libpcmkm.so with extra defines: tools/build_variant.sh NAME -DFLAG ...
# -> tools/ab/lib_NAME.so (tools/ab/ travels to the GPU box; load it with PCM_SO=tools/ab/lib_NAME.so)
# The translation units are _lib.UNITS, read from _lib.py (needs python3) so the two lists cannot drift apart.
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p tools/ab
P=3d-point-cloud-multiday-imagery_amd
# one unit per line, relative to the repository root, so that a checkout path with spaces works
mapfile -t units < <(python3 -c "import os, runpy; print('\n'.join(os.path.relpath(u) for u in runpy.run_path('$P/_lib.py')['UNITS']))")
[ ${#units[@]} -gt 0 ]
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I include "$@" \
  -o "tools/ab/lib_$name.so" "${units[@]}"
