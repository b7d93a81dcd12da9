// iou_grad.h -- dIoU/dbox of one pair of 2D boxes, shared by gnms_iou2d_backward (iou_backward.hip) and the sparse
// box-gradient kernel of the masked-group layer (nms_backward_kernels.h).  Both callers go through the SAME two functions with the
// same operand roles (a = the row box, b = the column box), so a pair's term is the same bits on either route.
//
// Reference: lib/core.py:499-508 differentiated by torch autograd.  torch's conventions: max / min split the gradient evenly between
// tied arguments, clamp(x, 0) passes the gradient at x = 0.  Plain IEEE fp32 (the library compiles with -ffp-contract=off), one true
// division per pair.
#pragma once
#include "gnms_common.h"

namespace gnms_iou_grad {

struct Pair {
    float w, h;          // clamped extents of the intersection
    float hx, wy;        // h where the x clamp passes the gradient (dx >= 0), else 0; w likewise for y
    float inter, uni;
    float rinv;          // 1 / uni^2
};

// a: the row box (area `aarea`), b: the column box.  The forward's operation order (iou_tile.h): uni = (area_a + area_b) - inter.
__device__ __forceinline__ Pair pair_of(const float4 a, float aarea, const float4 b, float barea) {
    Pair p;
    const float dx = fminf(a.z, b.z) - fmaxf(a.x, b.x);
    const float dy = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    p.w = fmaxf(dx, 0.0f);
    p.h = fmaxf(dy, 0.0f);
    p.hx = dx >= 0.0f ? p.h : 0.0f;
    p.wy = dy >= 0.0f ? p.w : 0.0f;
    p.inter = p.w * p.h;
    p.uni = (aarea + barea) - p.inter;
    p.rinv = 1.0f / (p.uni * p.uni);
    return p;
}

__device__ __forceinline__ float box_area(const float4 v) { return (v.z - v.x) * (v.w - v.y); }

// the share of a tied max (lower edges: s > o) or min (upper edges: s < o) that goes to `s`
__device__ __forceinline__ float share_lo(float s, float o) { return s > o ? 1.0f : (s == o ? 0.5f : 0.0f); }
__device__ __forceinline__ float share_hi(float s, float o) { return s < o ? 1.0f : (s == o ? 0.5f : 0.0f); }

__device__ __forceinline__ float coord_term(float d_inter, float d_area, const Pair& p) {
    return (d_inter * p.uni - p.inter * (d_area - d_inter)) * p.rinv;
}

// acc[c] += g * dIoU/d(s.c) for the four coordinates of `s`, one box of the pair `p`; `o` is the other box.  A cotangent of exactly 0
// contributes nothing, whatever the pair (torch would give 0 * NaN for a degenerate one).
__device__ __forceinline__ void add_box_grad(const float4 s, const float4 o, const Pair& p, float g, float (&acc)[4]) {
    const float sw = s.z - s.x, sh = s.w - s.y;
    const float t0 = g * coord_term(-(share_lo(s.x, o.x) * p.hx), -sh, p);
    const float t1 = g * coord_term(-(share_lo(s.y, o.y) * p.wy), -sw, p);
    const float t2 = g * coord_term(share_hi(s.z, o.z) * p.hx, sh, p);
    const float t3 = g * coord_term(share_hi(s.w, o.w) * p.wy, sw, p);
    const bool live = g != 0.0f;
    acc[0] += live ? t0 : 0.0f;
    acc[1] += live ? t1 : 0.0f;
    acc[2] += live ? t2 : 0.0f;
    acc[3] += live ? t3 : 0.0f;
}

}  // namespace gnms_iou_grad
