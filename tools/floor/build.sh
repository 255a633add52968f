#!/bin/bash
# Builds tools/floor/libfloor.so (measurement aid; the .so is git-ignored and travels to the GPU box with the snapshot).
# HIPCC and ARCH as in ppq_amd/csrc/Makefile.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
[ libfloor.so -nt floor_kernels.hip ] || "$HIPCC" --offload-arch="$ARCH" -O3 -std=c++17 -fPIC -shared -o libfloor.so floor_kernels.hip
echo built tools/floor/libfloor.so
