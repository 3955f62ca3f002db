#!/bin/bash
# A/B builds of the attention kernels: libvspike_<name>.so = the in-tree objects with one unit (attn_fwd.hip,
# attn_bwd.hip, attn_f32.hip, or a scratch copy of one) recompiled with extra flags.
# usage: build_attn_variant.sh <name> <src.hip> [flags...]     e.g.  stamp video-spike_amd/csrc/attn_fwd.hip -DVS_STAMP
# A scratch copy keeps the name of the unit it replaces (its object is the one left out of the link).
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1; src=$2; shift 2
B=video-spike_amd/vspike/_build
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I include -I video-spike_amd/csrc -munsafe-fp-atomics"
unit=$(basename "$src" .hip)
OTHERS=$(ls $B/*.o | grep -v "/$unit.o")
/opt/rocm/bin/hipcc $F "$@" -c "$src" -o /tmp/vs_var_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/libvspike_$name.so $OTHERS /tmp/vs_var_$name.o -lpthread -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
echo "built $B/libvspike_$name.so"
