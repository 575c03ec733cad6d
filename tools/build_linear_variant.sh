#!/bin/bash
# Build a library variant of one of the matcher's kernel files (A/B and ablation experiments; never
# shipped): SRC=linear (default: the projections), ffn, assign or glue -> csrc/lightglue_$SRC.hip
#   [SRC=ffn] tools/build_linear_variant.sh <name> [extra hipcc flags, e.g. -DLG_FR_STAMPS]  -> lib/ab/libmha_hd64_<name>.so
# lib/ab/ travels to the GPU box (lib/exp/ does not); delete it when the experiment is done.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../lightglue-with-flashattentionv2-tensorrt_amd"
mkdir -p lib/ab
make -s lib/libmha_hd64.so
S=${SRC:-linear}
# (the Makefile's flags for each source: the glue kernels without the device flags)
if [ "$S" = glue ]; then DEV=""; else DEV="-mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans"; fi
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $DEV "$@" \
      -I../include -Icsrc -c csrc/lightglue_$S.hip -o lib/ab/var_$NAME.o
OBJ=$(make -s print-objs)
hipcc --offload-arch=gfx950 -shared -fPIC ${OBJ/lib\/obj\/lightglue_$S.o/lib\/ab\/var_$NAME.o} -o lib/ab/libmha_hd64_$NAME.so
rm -f lib/ab/var_$NAME.o
echo lib/ab/libmha_hd64_$NAME.so
