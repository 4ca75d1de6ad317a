#!/bin/bash
# Device assembly of the library's kernels for gfx950, with the code-generation flags of pisces_amd/build.py:  tools/isa.sh out.s [-DFLAG ...]
out=$1; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mllvm -amdgpu-kernarg-preload-count=16 --cuda-device-only -S -x hip "$@" pisces_amd/csrc/pisces_hip.hip -o "$out"
