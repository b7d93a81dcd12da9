#!/bin/bash
# Developer build with the s_memtime phase markers (GNMS_TIMING) in a library of its own: build/timing/libgroomed_nms_hip.so = the NMS layer's
# units (nms_layer.hip and the nms_tail_*.hip / nms_tail_write_*.hip units, which hold the marked kernels) recompiled with -DGNMS_TIMING + the
# production objects of every other translation unit.  Use: GNMS_LIB_PATH=build/timing/libgroomed_nms_hip.so
# GNMS_BINDING=ctypes python tools/phase_ticks.py ...
set -e
cd "$(dirname "$0")/.."
mkdir -p build/timing
C=groomed_nms_amd/csrc
LAYER="nms_layer nms_tail_matrix nms_tail_boxes nms_tail_records nms_tail_write_boxes nms_tail_write_records"
pids=""
for u in $LAYER; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function -DGNMS_TIMING $EXTRA -c $C/$u.hip -o build/timing/$u.o &
    pids="$pids $!"
done
for p in $pids; do wait $p; done
OTHERS=$(ls $C/*.o | grep -v -E "/($(echo $LAYER | tr ' ' '|'))\.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/timing/libgroomed_nms_hip.so $(for u in $LAYER; do echo build/timing/$u.o; done) $OTHERS
ls -la build/timing/libgroomed_nms_hip.so
