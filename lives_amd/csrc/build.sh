#!/bin/bash
# Build liblivesgpu.so (gfx950 code objects only) in-tree: lives_amd/liblivesgpu.so
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -amdgpu-mfma-vgpr-form: MFMA results in VGPRs (no v_accvgpr_read per accumulator in the VALU-bound chain kernel)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form ${LGPU_EXTRA_FLAGS}"
OBJ=build
mkdir -p $OBJ
pids=()
for f in runtime swizzle yuv effects resize stencil palette pixbuf fused flat flat_select flat_luma; do
  stale=
  case $f in yuv|flat|flat_select|flat_luma|pixbuf) [ k2_walk.h -nt $OBJ/$f.o ] && stale=1 ;; esac      # K2's chroma walk, shared by the five
  case $f in flat|flat_select|flat_luma) { [ flat_walk.h -nt $OBJ/$f.o ] || [ flat_plan.h -nt $OBJ/$f.o ]; } && stale=1 ;; esac      # the unscaled forms' device text and host plan
  case $f in effects|flat_select) [ select_pred.h -nt $OBJ/$f.o ] && stale=1 ;; esac         # the iris and dissolve predicates
  case $f in flat_select) [ ../../include/lives_gpu_select.h -nt $OBJ/$f.o ] && stale=1 ;; esac
  case $f in effects|flat_luma) [ luma_pred.h -nt $OBJ/$f.o ] && stale=1 ;; esac             # the luma overlays' predicate
  case $f in flat_luma) [ ../../include/lives_gpu_luma.h -nt $OBJ/$f.o ] && stale=1 ;; esac
  if [ ! -f $OBJ/$f.o ] || [ $f.hip -nt $OBJ/$f.o ] || [ lgpu_common.h -nt $OBJ/$f.o ] || [ ../../include/lives_gpu.h -nt $OBJ/$f.o ] || [ -n "$stale" ]; then
    $HIPCC $FLAGS -c $f.hip -o $OBJ/$f.o &
    pids+=($!)
  fi
done
# the layer seam's units (layer_seam.cpp and seam_*.cpp) share the internal headers seam_*.h: a newer one rebuilds them all
for f in host_tables layer_seam seam_weed seam_resident seam_lazy dist; do
  stale=
  case $f in layer_seam|seam_*) for h in seam_*.h ../../include/lives_gpu_layer.h; do [ $h -nt $OBJ/$f.o ] && stale=1; done ;; esac
  if [ -f $f.cpp ] && { [ ! -f $OBJ/$f.o ] || [ $f.cpp -nt $OBJ/$f.o ] || [ ../../include/lives_gpu.h -nt $OBJ/$f.o ] || [ -n "$stale" ]; }; then
    g++ -O2 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -Wall -c $f.cpp -o $OBJ/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../liblivesgpu.so $OBJ/*.o -ldl -Wl,-soname,liblivesgpu.so
echo "built $(cd .. && pwd)/liblivesgpu.so"
