#!/bin/bash
# Build libpanonerf_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../libpanonerf_hip.so
FLAGS="$PN_EXTRA --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
OBJS=""
for f in pn_gemm pn_render pn_mlp pn_chain pn_wgrad pn_metrics pn_geometry pn_lighting pn_ibl pn_views pn_cameras pn_inpaint pn_data pn_objects pn_bvh pn_textures pn_atlas pn_relight pn_emitters pn_fusion pn_meshops pn_meshdist pn_winding pn_volume; do
  deps="$f.hip pn_common.h pn_tri.h pn_rays.h ../../include/panonerf_hip.h"
  case $f in pn_lighting|pn_ibl|pn_objects|pn_emitters|pn_volume) deps="$deps pn_probes.h";; esac  # the probe view, SH basis and tile walk
  case $f in pn_emitters|pn_meshops) deps="$deps pn_unionfind.h";; esac  # one union-find loop for pixels and mesh vertices
  case $f in pn_meshdist|pn_winding) deps="$deps pn_mesh64.h";; esac  # fp64 vectors and the face loader of the mesh queries
  case $f in pn_objects|pn_bvh|pn_meshdist|pn_winding) deps="$deps pn_bvh_walk.h";; esac  # the node row, the LDS stack and the ordered walk
  case $f in pn_chain|pn_wgrad) deps="$deps pn_chain.h";; esac  # the two kernel families of the fused MLP share it
  stale=0
  for d in $deps; do
    if [ ! -f "$f.o" ] || [ "$d" -nt "$f.o" ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then /opt/rocm/bin/hipcc $FLAGS -c "$f.hip" -o "$f.o"; fi
  OBJS="$OBJS $f.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS
echo "built $OUT"
