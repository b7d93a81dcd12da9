// bev_clip.h -- the exact area of the intersection of two convex quadrilaterals in float64 (Sutherland-Hodgman, fully unrolled), shared
// by iou3d_exact.hip (lib/core.py:246-302) and kitti_eval.hip (the devkit's groundBoxOverlap / box3DOverlap).  See iou3d_exact.hip's
// header comment for the choice of the algorithm and its conditioning.
#pragma once
#include <hip/hip_runtime.h>

namespace gnms_bev {

// cross(u, v) of two (x, z) vectors.  Products commute and x - y == -(y - x) in IEEE: cross(u, v) == -cross(v, u) exactly.
__device__ __forceinline__ double cross2(double ux, double uz, double vx, double vz) { return ux * vz - uz * vx; }

// twice the signed area of the quad, fanned from vertex 0 -- the products and the sum the shoelace of intersection_area forms for a
// box against an identical box (whose polygon is the box itself, vertex 0 at the origin), so that I == area exactly there
template <typename T>
__device__ __forceinline__ double twice_area(const T (&vx)[4], const T (&vz)[4]) {
    const double ox = (double)vx[0], oz = (double)vz[0];
    const double x1 = (double)vx[1] - ox, z1 = (double)vz[1] - oz, x2 = (double)vx[2] - ox, z2 = (double)vz[2] - oz;
    const double x3 = (double)vx[3] - ox, z3 = (double)vz[3] - oz;
    return cross2(x2, z2, x3, z3) + cross2(x1, z1, x2, z2);
}

// One Sutherland-Hodgman step: the polygon (px, pz) of n <= NIN vertices clipped to the left of the line through (ax, az) along
// (ex, ez).  Fully unrolled: every index is a compile-time constant, the output position is a select chain -- registers, no scratch.
// On the line counts as inside, so an edge shared with the clip line is kept once.
template <int NIN>
__device__ __forceinline__ int clip_step(const double (&px)[NIN], const double (&pz)[NIN], int n, double ax, double az, double ex,
                                         double ez, double (&qx)[NIN + 1], double (&qz)[NIN + 1]) {
    double f[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) f[i] = cross2(ex, ez, px[i] - ax, pz[i] - az);      // > 0: left of the line, inside
#pragma unroll
    for (int k = 0; k <= NIN; ++k) { qx[k] = 0.0; qz[k] = 0.0; }
    int m = 0;
    auto emit = [&](double x, double z) {
#pragma unroll
        for (int k = 0; k <= NIN; ++k) {
            if (k == m) { qx[k] = x; qz[k] = z; }
        }
        ++m;
    };
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        if (i < n) {
            const bool wrap = i + 1 >= n;
            const double nx = wrap ? px[0] : px[i + 1 < NIN ? i + 1 : 0];
            const double nz = wrap ? pz[0] : pz[i + 1 < NIN ? i + 1 : 0];
            const double fn = wrap ? f[0] : f[i + 1 < NIN ? i + 1 : 0];
            const double fc = f[i];
            if (fc >= 0.0 && fn >= 0.0) {
                emit(nx, nz);
            } else if (fc >= 0.0 || fn >= 0.0) {                                   // the edge crosses the line
                const double t = fc / (fc - fn);
                emit(px[i] + t * (nx - px[i]), pz[i] + t * (nz - pz[i]));
                if (fn >= 0.0) emit(nx, nz);
            }
        }
    }
    return m;
}

// B's half-plane j applied to the polygon (a repeated vertex of B bounds nothing: the polygon passes through unchanged)
template <int NIN>
__device__ __forceinline__ int clip_by(const double (&px)[NIN], const double (&pz)[NIN], int n, const double (&bx)[4],
                                       const double (&bz)[4], int j, double (&qx)[NIN + 1], double (&qz)[NIN + 1]) {
    const double ex = bx[(j + 1) & 3] - bx[j], ez = bz[(j + 1) & 3] - bz[j];
    if (ex == 0.0 && ez == 0.0) {
#pragma unroll
        for (int k = 0; k < NIN; ++k) { qx[k] = px[k]; qz[k] = pz[k]; }
        qx[NIN] = 0.0; qz[NIN] = 0.0;
        return n;
    }
    return clip_step<NIN>(px, pz, n, bx[j], bz[j], ex, ez, qx, qz);
}

// area of A n B, both counter-clockwise with coordinates relative to A's vertex 0: A clipped by B's 4 half-planes (at most 8
// vertices), then the shoelace sum.  For B == A the polygon is A itself and the sum forms the products of twice_area: I == area.
__device__ __forceinline__ double intersection_area(const double (&ax)[4], const double (&az)[4], const double (&bx)[4], const double (&bz)[4]) {
    double x5[5], z5[5], x6[6], z6[6], x7[7], z7[7], x8[8], z8[8];
    int n = clip_by<4>(ax, az, 4, bx, bz, 0, x5, z5);
    n = clip_by<5>(x5, z5, n, bx, bz, 1, x6, z6);
    n = clip_by<6>(x6, z6, n, bx, bz, 2, x7, z7);
    n = clip_by<7>(x7, z7, n, bx, bz, 3, x8, z8);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < n) {
            const bool wrap = k + 1 >= n;
            const double nx = wrap ? x8[0] : x8[k + 1 < 8 ? k + 1 : 0], nz = wrap ? z8[0] : z8[k + 1 < 8 ? k + 1 : 0];
            s = s + cross2(x8[k], z8[k], nx, nz);
        }
    }
    return 0.5 * s;
}

}  // namespace gnms_bev
