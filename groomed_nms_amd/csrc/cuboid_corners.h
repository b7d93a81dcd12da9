// cuboid_corners.h -- get_corners_of_cuboid for one box, ONE definition shared by the corner / record kernels of iou_kernels.hip
// and the from-params prologue of iou3d_exact.hip, so that "params -> corners -> exact IoU" and "params -> exact IoU" see the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "iou3d_pair.h"

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

// per-box axis-aligned record of the corners (the layout stands in iou_kernels.hip): ONE definition, so that the 3D overlap backward
// (iou3d_grad.h) decides ties and clamps on the very floats the forward saw
__device__ __forceinline__ void aabb_record(const float (&cx)[8], const float (&cy)[8], const float (&cz)[8], float* rec) {
    float mnx = cx[0], mxx = cx[0], mny = cy[0], mxy = cy[0], mnz = cz[0], mxz = cz[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        mnx = fminf(mnx, cx[k]); mxx = fmaxf(mxx, cx[k]);
        mny = fminf(mny, cy[k]); mxy = fmaxf(mxy, cy[k]);
        mnz = fminf(mnz, cz[k]); mxz = fmaxf(mxz, cz[k]);
    }
    float vol = ((mxx - mnx) * (mxy - mny)) * (mxz - mnz);
    float x0 = fminf(fminf(cx[2], cx[3]), fminf(cx[6], cx[7])), x1 = fmaxf(fmaxf(cx[2], cx[3]), fmaxf(cx[6], cx[7]));
    float z0 = fminf(fminf(cz[2], cz[3]), fminf(cz[6], cz[7])), z1 = fmaxf(fmaxf(cz[2], cz[3]), fmaxf(cz[6], cz[7]));
    rec[0] = vol; rec[1] = mny; rec[2] = mxy; rec[3] = x0; rec[4] = x1; rec[5] = z0; rec[6] = z1;
    rec[7] = (x1 - x0) * (z1 - z0);
    rec[8] = x1 - x0; rec[9] = mxy - mny; rec[10] = z1 - z0;                      // extents, used by the fast NMS-overlap kernel
    rec[11] = gnms_iou3d::record_bad_flag(x0, x1, mny, mxy, z0, z1, rec[8], rec[9], rec[10]);   // 0 = sane (iou3d_pair.h)
}

}  // namespace gnms_geom
