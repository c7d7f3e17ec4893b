#!/bin/bash
# Builds one library per cache-policy variant of the mapping kernel's per-wave state (README.md in this directory).
# Needs state_policy.patch applied and a finished `make` (the other objects are linked as they are).
# usage: scripts/experiments/state_policy/build_variants.sh name:"-DCMX_V_ST=kPolNt" ...   -> build/libs/<name>.so, build/sp/<name>/
set -e
ROOT="$(cd "$(dirname "$0")/../../.." && pwd)"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form=1"
cd "$ROOT/comap_amd/csrc"
mkdir -p "$ROOT/build/libs"
for v in "$@"; do
  name=${v%%:*}; defs=${v#*:}
  d="$ROOT/build/sp/$name"; mkdir -p "$d"
  ( $HIPCC $FLAGS $defs -c cmx_map.hip -o "$d/cmx_map.o" -save-temps=obj -Rpass-analysis=kernel-resource-usage 2> "$d/resource_usage.txt" &&
    $HIPCC --offload-arch=gfx950 -shared -fPIC "$d/cmx_map.o" $(ls _obj/*.o | grep -v '/cmx_map\.o$') -o "$ROOT/build/libs/$name.so" &&
    echo "built $name" || echo "FAILED $name" ) &
done
wait
