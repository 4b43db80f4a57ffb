#!/bin/bash
# tools/build_ab.sh <name> [extra hipcc flags]  -- build a variant of the library into gpurun_tmp/lib_<name>.so (for tools/ab_lib.sh);
# e.g.  tools/build_ab.sh new ; tools/build_ab.sh probe -DMGPT_ABL_GEMM_16X16  (the library's remaining -D switches: tools/README.md)
cd "$(dirname "$0")/.."
N=$1; shift
B=/tmp/ab_build_$N; mkdir -p $B gpurun_tmp
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable -Wno-unused-but-set-variable $*"
pids=()
SRCS=$(python -c "from mapf_gpt_amd.build import SOURCES; print(' '.join(s[:-4] for s in SOURCES))") || exit 1     # the translation units build.py compiles
for s in $SRCS; do
  /opt/rocm/bin/hipcc $FLAGS -c mapf_gpt_amd/csrc/$s.hip -o $B/$s.o & pids+=($!)
done
for p in "${pids[@]}"; do wait $p || exit 1; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o gpurun_tmp/lib_$N.so $B/*.o && ls -la gpurun_tmp/lib_$N.so
