#!/bin/bash
# usage: tools/build_variant.sh <suffix> <extra hipcc flags...>: the two files of the fused MLP (pn_chain.hip, pn_wgrad.hip) with extra
# defines, linked with the other objects of csrc/build.sh (run that first) -> libpanonerf_hip_<suffix>.so
set -e
cd "$(dirname "$0")/../pano-nerf_amd/csrc"
sfx=$1; shift
objs=""
for src in pn_*.hip; do  # (build.sh links one object per .hip of this directory)
  f=${src%.hip}
  case $f in
    pn_chain|pn_wgrad)
      /opt/rocm/bin/hipcc "$@" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -c $src -o /tmp/${f}_$sfx.o
      objs="$objs /tmp/${f}_$sfx.o";;
    *) objs="$objs $f.o";;
  esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libpanonerf_hip_$sfx.so $objs
echo built $sfx
