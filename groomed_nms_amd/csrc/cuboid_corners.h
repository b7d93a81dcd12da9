// cuboid_corners.h -- get_corners_of_cuboid for one box, ONE definition shared by the corner / record kernels of iou_kernels.hip
// and the from-params prologue of iou3d_exact.hip, so that "params -> corners -> exact IoU" and "params -> exact IoU" see the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace gnms_geom {

// get_corners_of_cuboid, lib/math_3d.py:364-435 (same operation order as oracle/gnms_oracle.c)
__device__ __forceinline__ void corners_of(const float* p, float (&cx)[8], float (&cy)[8], float (&cz)[8]) {
    const float x = p[0], y = p[1], z = p[2], w = p[3], h = p[4], l = p[5], ry = p[6];
    const float c = cosf(ry), s = sinf(ry);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool xh = (k == 1) | (k == 3) | (k == 5) | (k == 6);   // :401
        const bool yh = (k == 2) | (k == 3) | (k == 6) | (k == 7);   // :402
        const bool zh = k >= 4;                                      // :403
        float bx = (xh ? l : 0.0f) - l / 2;
        float by = (yh ? h : 0.0f) - h / 2;
        float bz = (zh ? w : 0.0f) - w / 2;
        float rx = c * bx + 0.0f * by + s * bz;                      // bmm(R, corners) :430
        float ryy = 0.0f * bx + 1.0f * by + 0.0f * bz;
        float rz = (-s) * bx + 0.0f * by + c * bz;
        cx[k] = rx + x; cy[k] = ryy + y; cz[k] = rz + z;             // :433-435
    }
}

}  // namespace gnms_geom
