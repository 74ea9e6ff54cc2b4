#!/bin/bash
# Same-box A/B/C/... timing, alternating runs of tools/time_ops.py: bash tools/abn.sh <rounds> <variant>...
# A variant is a build_ab/<name>/lib.so name (tools/build_variant.sh) or the path of a library; ARGS="<time_ops args>" replaces the default.
N=$1; shift
ARGS=${ARGS:---only both --iters 60}
for i in $(seq $N); do
    for v in "$@"; do
        lib=$v; [ -f "$lib" ] || lib=build_ab/$v/lib.so
        ABL_NAME=$v RWKV_AMD_LIB=$lib RWKV_AMD_NO_SELFTEST=1 python tools/time_ops.py $ARGS 2>&1 | grep -v amdgpu.ids
    done
done
