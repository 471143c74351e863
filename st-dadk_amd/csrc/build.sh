#!/bin/bash
# Builds st-dadk_amd/lib/libstdadk.so for gfx950 (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
mkdir -p ../lib obj
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function ${STDADK_EXTRA_FLAGS:-}"
# an object is out of date when its source, ANY header of this directory or the public header is newer than it
stale() {  # stale <object> <source>
  local dep
  for dep in "$2" *.h ../../include/stdadk.h; do
    if [ ! -f "$1" ] || [ "$dep" -nt "$1" ]; then return 0; fi
  done
  return 1
}
pids=()
for f in rbf_build gemm_f32 mlp optim window tail loss knots step_finish fused_step dw_all sparsity eval grid_score quantile_diag variogram basis_diag conformal knn knn_cells krige gmm kmeans kmeanspp; do
  if stale obj/$f.o $f.hip; then
    $HIPCC $FLAGS -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
if [ ! -f obj/api.o ] || [ api.cpp -nt obj/api.o ] || [ ../../include/stdadk.h -nt obj/api.o ]; then
  $HIPCC $FLAGS -x hip -c api.cpp -o obj/api.o &
  pids+=($!)
fi
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC -shared -fPIC --offload-arch=gfx950 obj/*.o -o ../lib/libstdadk.so
echo "built $(cd ../lib && pwd)/libstdadk.so"
