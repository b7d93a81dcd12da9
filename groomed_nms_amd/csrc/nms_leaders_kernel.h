// nms_leaders_kernel.h -- K3 as a launch of its own: leaders_kernel, the one non-template __global__ function of the leader scan
// (nms_scan_kernels.h).  In a header of its own because the build treats a non-template kernel that an including unit does not launch as an
// error: included by the two units that launch it, nms_layer.hip (through nms_layer_kernels.h) and classic_nms.hip, while the units that
// only borrow the scan's bodies (the tails: nms_tail_*.hip) include nms_scan_kernels.h alone.
#pragma once
#include "nms_scan_kernels.h"

namespace gnms {
namespace {   // internal linkage: the header is included by several translation units

__global__ __launch_bounds__(1024) void leaders_kernel(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, int sym, int B, int spw,
                                                       const u64* __restrict__ ext0 = nullptr) {
    int b;
    leaders_chain(N, counts, ws, L, B, spw, (int)blockIdx.x, sym, &b, nullptr, 0, 0.0f, 0.0f, 0, 0, ext0);
}

}  // namespace
}  // namespace gnms
