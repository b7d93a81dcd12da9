// iou3d_grad.h -- d overlap3d / d cuboid of one pair, shared by gnms_iou3d_backward (iou3d_backward.hip) and the sparse
// cuboid-gradient kernel of the masked-group layer (nms_backward_kernels.h).  Both callers go through the SAME functions with the same
// operand roles (a = the row box, b = the column box), so a pair's term is the same bits on either route.
//
// Two stages.  Stage 2 (pair_of, add_extent_grad): the derivative of the overlap w.r.t. the six axis-aligned extents
// E = (x0, x1, y0, y1, z0, z1) of one box of the pair, on the float32 extents the forward saw (aabb_record, cuboid_corners.h).
// Stage 1 (params_grad): the sum of a box's extent gradients carried to its seven parameters, ONCE per box.
//
// Reference: lib/math_3d.py:364-435 + lib/core.py:305-421 (+ lib/loss/rpn_3d.py:781) differentiated by torch autograd.  torch's
// conventions: an elementwise max / min of the two boxes' edges splits the gradient evenly between tied arguments; the x and z
// intersection extents come from clamp(., 0), which passes the gradient at 0; the y intersection extent and the three hull extents
// come from torch.max(zeros, .), which gives 1/2 at exactly 0.  Plain IEEE fp32 (the library compiles with -ffp-contract=off), two
// true divisions per pair.
#pragma once
#include "cuboid_corners.h"

namespace gnms_iou3d_grad {

struct Rec {             // what the backward reads of a box's record: the first seven floats (u | v of iou3d_pair.h)
    float x0, x1, y0, y1, z0, z1, vol;
};
__device__ __forceinline__ Rec rec_of(const float4 u, const float4 v) {
    Rec r;
    r.vol = u.x; r.y0 = u.y; r.y1 = u.z; r.x0 = u.w; r.x1 = v.x; r.z0 = v.y; r.z1 = v.z;
    return r;
}

// the record of one cuboid from its seven parameters: the forward's own floats (corners_of + aabb_record)
__device__ __forceinline__ void record_of_params(const float* __restrict__ p, float4& u, float4& v, float4& e) {
    float cx[8], cy[8], cz[8], r[gnms_iou3d::kRec];
    gnms_geom::corners_of(p, cx, cy, cz);
    gnms_geom::aabb_record(cx, cy, cz, r);
    u = make_float4(r[0], r[1], r[2], r[3]);
    v = make_float4(r[4], r[5], r[6], r[7]);
    e = make_float4(r[8], r[9], r[10], r[11]);
}

struct Pair {
    float pi[3];         // d I / d (the intersection extent of axis x, y, z), the clamp's factor included
    float ph[3];         // d H / d (the hull extent of axis x, y, z), likewise
    float I, U, H;
    float ru, rh;        // 1 / U^2, 1 / H^2
};

// factor of max(zeros, d) at d: 1, 1/2 at exactly 0, 0
__device__ __forceinline__ float pass_half(float d) { return d > 0.0f ? 1.0f : (d == 0.0f ? 0.5f : 0.0f); }

// a: the row box, b: the column box.  The forward's operation order (nms_overlap3d_exact): I = (ex ez) ey, U = (vol_a + vol_b) - I,
// H = (hx hy) hz.
__device__ __forceinline__ Pair pair_of(const Rec& a, const Rec& b) {
    Pair p;
    const float dx = fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0);
    const float dy = fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0);
    const float dz = fminf(a.z1, b.z1) - fmaxf(a.z0, b.z0);
    const float ex = fmaxf(dx, 0.0f), ey = fmaxf(dy, 0.0f), ez = fmaxf(dz, 0.0f);
    const float Dx = fmaxf(a.x1, b.x1) - fminf(a.x0, b.x0);
    const float Dy = fmaxf(a.y1, b.y1) - fminf(a.y0, b.y0);
    const float Dz = fmaxf(a.z1, b.z1) - fminf(a.z0, b.z0);
    const float hx = fmaxf(Dx, 0.0f), hy = fmaxf(Dy, 0.0f), hz = fmaxf(Dz, 0.0f);
    p.pi[0] = dx >= 0.0f ? ez * ey : 0.0f;                            // clamp(., 0): passes at 0
    p.pi[1] = pass_half(dy) * (ex * ez);                              // torch.max(zeros, .): 1/2 at 0
    p.pi[2] = dz >= 0.0f ? ex * ey : 0.0f;
    p.ph[0] = pass_half(Dx) * (hy * hz);
    p.ph[1] = pass_half(Dy) * (hx * hz);
    p.ph[2] = pass_half(Dz) * (hx * hy);
    p.I = (ex * ez) * ey;
    p.U = (a.vol + b.vol) - p.I;
    p.H = (hx * hy) * hz;
    p.ru = 1.0f / (p.U * p.U);
    p.rh = 1.0f / (p.H * p.H);
    return p;
}

// the share of a tied max (s > o) or min (s < o) that goes to `s`
__device__ __forceinline__ float share_gt(float s, float o) { return s > o ? 1.0f : (s == o ? 0.5f : 0.0f); }
__device__ __forceinline__ float share_lt(float s, float o) { return s < o ? 1.0f : (s == o ? 0.5f : 0.0f); }

// METHOD as gnms_iou3d_from_params: 0  I/U;  1  I/U - (H - U)/H;  2  0.5 (1 + that).  Two quotient rules, dU = dvol - dI.
template <int METHOD>
__device__ __forceinline__ float edge_term(float d_i, float d_vol, float d_h, const Pair& p) {
    const float d_u = d_vol - d_i;
    const float qi = (d_i * p.U - p.I * d_u) * p.ru;
    if (METHOD == 0) return qi;
    const float qh = (d_u * p.H - p.U * d_h) * p.rh;
    return METHOD == 1 ? qi + qh : 0.5f * (qi + qh);
}

// acc[k] += g * d overlap / d(s.E_k) for the six extents (x0, x1, y0, y1, z0, z1) of `s`, one box of the pair `p`; `o` is the other
// box.  A cotangent of exactly 0 contributes nothing, whatever the pair (torch would give 0 * NaN for a degenerate one).
template <int METHOD>
__device__ __forceinline__ void add_extent_grad(const Rec& s, const Rec& o, const Pair& p, float g, float (&acc)[6]) {
    const float lx = s.x1 - s.x0, ly = s.y1 - s.y0, lz = s.z1 - s.z0;
    const float ax = ly * lz, ay = lx * lz, az = lx * ly;             // d vol / d (an upper edge)
    float t[6];
    // a lower edge: the max of the intersection's lower edges (s > o), the min of the hull's (s < o); an upper edge the other way round
    t[0] = g * edge_term<METHOD>(-(share_gt(s.x0, o.x0) * p.pi[0]), -ax, -(share_lt(s.x0, o.x0) * p.ph[0]), p);
    t[1] = g * edge_term<METHOD>(share_lt(s.x1, o.x1) * p.pi[0], ax, share_gt(s.x1, o.x1) * p.ph[0], p);
    t[2] = g * edge_term<METHOD>(-(share_gt(s.y0, o.y0) * p.pi[1]), -ay, -(share_lt(s.y0, o.y0) * p.ph[1]), p);
    t[3] = g * edge_term<METHOD>(share_lt(s.y1, o.y1) * p.pi[1], ay, share_gt(s.y1, o.y1) * p.ph[1], p);
    t[4] = g * edge_term<METHOD>(-(share_gt(s.z0, o.z0) * p.pi[2]), -az, -(share_lt(s.z0, o.z0) * p.ph[2]), p);
    t[5] = g * edge_term<METHOD>(share_lt(s.z1, o.z1) * p.pi[2], az, share_gt(s.z1, o.z1) * p.ph[2], p);
    const bool live = g != 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += live ? t[k] : 0.0f;
}

// Stage 1.  ex = |c| l + |s| w, ez = |s| l + |c| w, x0,1 = x -+ ex/2, y0,1 = y -+ h/2, z0,1 = z -+ ez/2 with c = cos ry, s = sin ry
// (the same cosf / sinf as corners_of).  sgn 0 = 0: where corners tie (ry = +-0 in float32) they share the gradient, d ry = 0 there.
__device__ __forceinline__ float sgn0(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ void params_grad(const float* __restrict__ p, const float (&G)[6], float (&d)[7]) {
    const float w = p[3], l = p[5], ry = p[6];
    const float c = cosf(ry), s = sinf(ry);
    const float ac = fabsf(c), as = fabsf(s), sc = sgn0(c), ss = sgn0(s);
    const float gx = G[1] - G[0], gz = G[5] - G[4];
    d[0] = G[0] + G[1];
    d[1] = G[2] + G[3];
    d[2] = G[4] + G[5];
    d[3] = (as * gx + ac * gz) * 0.5f;
    d[4] = (G[3] - G[2]) * 0.5f;
    d[5] = (ac * gx + as * gz) * 0.5f;
    d[6] = (((c * ss) * w - (s * sc) * l) * gx + ((c * ss) * l - (s * sc) * w) * gz) * 0.5f;
}

}  // namespace gnms_iou3d_grad
