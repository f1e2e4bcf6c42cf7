#!/bin/bash
# A/B builds of the library with extra -D flags:  scripts/build_variant.sh <name> "<flags>"  -> rpt_amd/lib/librptgpu_<name>.so
# (use with RPTGPU_LIB=$PWD/rpt_amd/lib/librptgpu_<name>.so; the kernel builds of every form of the persistent kernel and the
# api_*.cpp files are rebuilt with the flags; the surface resolve's kernels, host_scene.o, kdbuild.o, particles.o, mesh_update.o
# and group_update.o are taken from the regular build).  NOEXT=1 skips the extended-shape builds (takes the regular ones).
# JOBS: compilations at a time (default 8).
set -e
NAME=$1; FLAGS=$2; JOBS=${JOBS:-8}
cd $(dirname $0)/../rpt_amd/csrc
make -s -j$JOBS
B=build/var_$NAME; mkdir -p $B
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
KERNELS="kernels_strict kernels_views_strict kernels_rays_strict kernels_vertices_strict"
KERNELS_EXT="kernels_strict_ext kernels_views_strict_ext kernels_rays_strict_ext kernels_vertices_strict_ext"
API="api_common api_scene api_render api_comm api_buffer api_particles api_aov api_rays api_probes api_views api_views_denoise api_occlusion api_hits api_surface api_vertices api_mesh api_group"
if [ -n "$NOEXT" ]; then for k in $KERNELS_EXT; do cp build/$k.o $B/; done; else KERNELS="$KERNELS $KERNELS_EXT"; fi
{
  for k in $KERNELS; do echo "$COMMON -ffp-contract=off $FLAGS -c $k.hip -o $B/$k.o"; done
  for a in $API; do echo "$COMMON -ffp-contract=off $FLAGS -x hip -c $a.cpp -o $B/$a.o"; done
} | xargs -P $JOBS -L 1 /opt/rocm/bin/hipcc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/librptgpu_$NAME.so \
  $(for k in $KERNELS $([ -n "$NOEXT" ] && echo $KERNELS_EXT) ; do echo $B/$k.o; done) $(for a in $API; do echo $B/$a.o; done) \
  build/kernels_surface_strict.o build/kernels_surface_strict_ext.o build/host_scene.o build/kdbuild.o build/particles.o build/mesh_update.o build/group_update.o
echo built ../lib/librptgpu_$NAME.so
