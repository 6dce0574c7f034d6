#!/bin/bash
# Build libnnr_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../libnnr_hip.so
FLAGS="${NNR_EXTRA_FLAGS} --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -Wno-pass-failed"
mkdir -p build
pids=()
compiled=""
kept=""
objs=""
# incremental: a source is recompiled when it, any header here or the public header is newer than its object (NNR_BUILD_FORCE=1: everything);
# what was compiled and what was kept is printed, so a caller can see which it got
newest_h=$(ls -t *.h ../../include/nnr_hip.h | head -1)
for f in gemm seq_plan lstm pool misc mhsa corpus dp gcn tape fuse sort cand_attn omap pers_attn kcnn hdc fim gru naml dssm sue_cluster topk bag; do
  [ -f $f.hip ] || continue
  objs="$objs build/$f.o"
  if [ "${NNR_BUILD_FORCE}" = "1" ] || [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ $newest_h -nt build/$f.o ]; then
    hipcc $FLAGS -c $f.hip -o build/$f.o &
    pids+=($!)
    compiled="$compiled $f"
  else
    kept="$kept $f"
  fi
done
for p in "${pids[@]}"; do wait $p; done
echo "compiled:${compiled:- (none)}; up to date:${kept:- (none)}"
# exactly the objects of the list: an object left in build/ by a source that was renamed or removed is not linked
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $objs -ldl
echo "built $(realpath $OUT)"
