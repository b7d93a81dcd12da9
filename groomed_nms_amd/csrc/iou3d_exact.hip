// iou3d_exact.hip -- the exact IoU of two rotated cuboids, lib/core.py:246-302 (iou3d), for gfx950 (MI355X).
//
// Reference: the bird's-eye-view footprint of a box is the polygon of its corners 7, 2, 3, 6 in (x, z) (:289-294); shapely intersects
// the two footprints (:296); the 3D intersection is that area times the overlap of the boxes' y ranges over all 8 corners (:282-287);
//   iou_bev = I / (area_a + area_b - I)            iou_3d = I * y_overlap / (vol - I * y_overlap)                          (:299-300)
// with vol = get_volume(a) + get_volume(b), the corner AABB volumes (:276-277, :452-456), when the caller passes none.
//
// Geometry in float64, like GEOS.  Footprints are convex quadrilaterals of either orientation (negative w / l flip it): each is
// normalised to counter-clockwise by the sign of its shoelace area.  Non-convex or self-intersecting quadrilaterals are not supported.
//
// Intersection area: A's footprint clipped by B's 4 half-planes (Sutherland-Hodgman, fully unrolled: at most 8 vertices in
// registers, every index a compile-time constant, no scratch), then the shoelace sum.  A point on a clip line counts as inside, so
// an edge shared by both footprints is kept once.  The output vertices lie on A's edges or on B's edge lines, so the ill-conditioned
// crossing of two nearly parallel edges moves a vertex ALONG the two nearly coincident lines and changes the area by a second-order
// sliver only (a form that sums the clipped edges of both footprints separately double-counts such edges: measured, rejected).
// Coordinates are taken relative to vertex 0 of A, so the cross products are of the size of the boxes, not of their distance to the
// origin.  A pair whose footprint area is 0 on either side has I = 0 exactly (two such boxes: 0/0 = NaN, as in the reference).
//
// Matrix kernel: one workgroup = 8 rows x 256 columns.  Each tile derives its box records itself (no workspace, capturable):
//   1. records -> LDS (the thread's column box, threads 0..7 also a row box);
//   2. reject: per pair, the xz-AABBs must overlap and, without iou_bev, the y ranges too; the value of every other pair (I = 0) goes
//      to the LDS output tile, the candidates to an LDS work list (ballot + one LDS atomic per wave and row);
//   3. clip: one lane per candidate; the value overwrites the tile entry;
//   4. the tile leaves as coalesced 16-byte non-temporal rows.
// Only the ~2 % of pairs that overlap pay for the float64 clip (iou3d_exact).
#include "gnms_common.h"
#include "iou_tile.h"
#include "cuboid_corners.h"
#include "bev_clip.h"

namespace {

using namespace gnms_bev;

constexpr int kTM = 8;                 // rows of a workgroup tile
constexpr int kTN = 256;               // columns of a workgroup tile == threads of a workgroup
constexpr int kBoxes = kTM + kTN;      // LDS record slots: rows first

// One box's footprint and extents, vertices in the input precision T (fp32 corners stay exact in fp32).
template <typename T>
struct Rec {
    T vx[4], vz[4];        // footprint, counter-clockwise
    T x0, x1, z0, z1;      // footprint AABB
    T y0, y1;              // y range over all 8 corners
    double area;           // footprint area
    double vol;            // volume_mode 0: area * y extent; 1: corner AABB volume (get_volume)
};

template <typename T>
__device__ __forceinline__ T tmin(T a, T b) { return a < b ? a : b; }
template <typename T>
__device__ __forceinline__ T tmax(T a, T b) { return a > b ? a : b; }

template <typename T>
__device__ __forceinline__ void make_rec(const T (&cx)[8], const T (&cy)[8], const T (&cz)[8], int volume_mode, Rec<T>& r) {
    // lib/core.py:289-294: polygon_order = [7, 2, 3, 6, 7], (x, z) after "set Z as Y"
    r.vx[0] = cx[7]; r.vx[1] = cx[2]; r.vx[2] = cx[3]; r.vx[3] = cx[6];
    r.vz[0] = cz[7]; r.vz[1] = cz[2]; r.vz[2] = cz[3]; r.vz[3] = cz[6];
    double s = twice_area(r.vx, r.vz);
    if (s < 0.0) {                                                   // clockwise: v0 v3 v2 v1
        T t = r.vx[1]; r.vx[1] = r.vx[3]; r.vx[3] = t;
        t = r.vz[1]; r.vz[1] = r.vz[3]; r.vz[3] = t;
        s = twice_area(r.vx, r.vz);
    }
    r.area = 0.5 * s;
    r.x0 = tmin(tmin(r.vx[0], r.vx[1]), tmin(r.vx[2], r.vx[3]));
    r.x1 = tmax(tmax(r.vx[0], r.vx[1]), tmax(r.vx[2], r.vx[3]));
    r.z0 = tmin(tmin(r.vz[0], r.vz[1]), tmin(r.vz[2], r.vz[3]));
    r.z1 = tmax(tmax(r.vz[0], r.vz[1]), tmax(r.vz[2], r.vz[3]));
    T y0 = cy[0], y1 = cy[0], ax0 = cx[0], ax1 = cx[0], az0 = cz[0], az1 = cz[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {                                    // :282-285 (np.min / np.max over the 8 corners)
        y0 = tmin(y0, cy[k]); y1 = tmax(y1, cy[k]);
        ax0 = tmin(ax0, cx[k]); ax1 = tmax(ax1, cx[k]);
        az0 = tmin(az0, cz[k]); az1 = tmax(az1, cz[k]);
    }
    r.y0 = y0; r.y1 = y1;
    if (volume_mode == 0) r.vol = r.area * ((double)y1 - (double)y0);
    else r.vol = (((double)ax1 - (double)ax0) * ((double)y1 - (double)y0)) * ((double)az1 - (double)az0);   // :452-456, np.prod
}

// ------------------------------------------------------------------------------------------------
// Matrix kernel.  A [B][M][3][8] corners (or [B][M][7] params), Bx likewise with N, outputs [B][M][ld].
// ------------------------------------------------------------------------------------------------
template <bool FROM_PARAMS>
__device__ __forceinline__ void load_rec(const float* __restrict__ src, size_t box, int volume_mode, Rec<float>& r) {
    float cx[8], cy[8], cz[8];
    if (FROM_PARAMS) {
        gnms_geom::corners_of(src + box * 7, cx, cy, cz);
    } else {
        const float* c = src + box * 24;
#pragma unroll
        for (int k = 0; k < 8; ++k) { cx[k] = c[k]; cy[k] = c[8 + k]; cz[k] = c[16 + k]; }
    }
    make_rec(cx, cy, cz, volume_mode, r);
}

struct TileLDS {
    float vx[4][kBoxes], vz[4][kBoxes];
    float y0[kBoxes], y1[kBoxes];
    float rx0[kTM], rx1[kTM], rz0[kTM], rz1[kTM];
    double area[kBoxes], vol[kBoxes];
    float out[2][kTM][kTN];            // [0] iou_bev, [1] iou_3d
    unsigned short list[kTM * kTN];    // candidate pairs, row * kTN + column
    int count;
};

__device__ __forceinline__ void put_rec(TileLDS& s, int slot, const Rec<float>& r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { s.vx[k][slot] = r.vx[k]; s.vz[k][slot] = r.vz[k]; }
    s.y0[slot] = r.y0; s.y1[slot] = r.y1;
    s.area[slot] = r.area; s.vol[slot] = r.vol;
}

template <bool FROM_PARAMS>
__global__ __launch_bounds__(kTN) void iou3d_exact_kernel(const float* __restrict__ A, const float* __restrict__ Bx, int M, int N,
                                                          int volume_mode, float* __restrict__ bev, float* __restrict__ i3, long ld,
                                                          int vec) {
    __shared__ TileLDS s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * kTN, r0 = blockIdx.y * kTM, img = blockIdx.z;
    const int col = c0 + tid;
    const bool cvalid = col < N;
    const bool want_bev = bev != nullptr;

    // 1. records.  Out-of-range boxes read the last valid box and never become candidates or leave the tile.
    Rec<float> c;
    load_rec<FROM_PARAMS>(Bx, (size_t)img * N + (cvalid ? col : N - 1), volume_mode, c);
    put_rec(s, kTM + tid, c);
    if (tid < kTM) {
        Rec<float> r;
        const int row = min(r0 + tid, M - 1);
        load_rec<FROM_PARAMS>(A, (size_t)img * M + row, volume_mode, r);
        put_rec(s, tid, r);
        s.rx0[tid] = r.x0; s.rx1[tid] = r.x1; s.rz0[tid] = r.z0; s.rz1[tid] = r.z1;
    }
    if (tid == 0) s.count = 0;
    __syncthreads();

    // 2. reject, defaults, work list
    for (int r = 0; r < kTM; ++r) {
        const float ry0 = s.y0[r], ry1 = s.y1[r];
        const double yov = fmax(0.0, (double)fminf(ry1, c.y1) - (double)fmaxf(ry0, c.y0));      // :286
        const double asum = c.area + s.area[r], vsum = s.vol[r] + c.vol;
        const bool xz = fmaxf(s.rx0[r], c.x0) < fminf(s.rx1[r], c.x1) && fmaxf(s.rz0[r], c.z0) < fminf(s.rz1[r], c.z1);
        const bool cand = cvalid && (r0 + r < M) && xz && s.area[r] > 0.0 && c.area > 0.0 && (want_bev || yov > 0.0);
        // I = 0: 0 / asum and (0 * yov) / (vsum - 0 * yov) without the divisions (asum, vsum >= 0 or NaN; yov >= 0)
        s.out[0][r][tid] = asum > 0.0 ? 0.0f : __builtin_nanf("");
        s.out[1][r][tid] = (vsum > 0.0 && yov < __builtin_inf()) ? 0.0f : __builtin_nanf("");
        const unsigned long long m = __ballot(cand);
        if (m) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&s.count, __popcll(m));
            base = __shfl(base, 0);
            if (cand) {
                const int pos = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                s.list[pos] = (unsigned short)(r * kTN + tid);
            }
        }
    }
    __syncthreads();

    // 3. clip: one lane per candidate
    const int count = s.count;
    for (int k = tid; k < count; k += kTN) {
        const int p = s.list[k], r = p / kTN, cs = kTM + (p % kTN);
        const double ox = (double)s.vx[0][r], oz = (double)s.vz[0][r];
        double ax[4], az[4], bx[4], bz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ax[q] = (double)s.vx[q][r] - ox; az[q] = (double)s.vz[q][r] - oz;
            bx[q] = (double)s.vx[q][cs] - ox; bz[q] = (double)s.vz[q][cs] - oz;
        }
        const double I = intersection_area(ax, az, bx, bz);                                     // :296
        const double yov = fmax(0.0, (double)fminf(s.y1[r], s.y1[cs]) - (double)fmaxf(s.y0[r], s.y0[cs]));
        const double I3 = yov * I;                                                               // :297
        s.out[0][r][p % kTN] = (float)(I / ((s.area[cs] + s.area[r]) - I));                      // :299
        s.out[1][r][p % kTN] = (float)(I3 / ((s.vol[r] + s.vol[cs]) - I3));                      // :300
    }
    __syncthreads();

    // 4. coalesced rows: wave w writes rows w, w + 4 of each requested output, lane = 4 columns
    const size_t img_off = (size_t)img * M * ld;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        float* dst = o == 0 ? bev : i3;
        if (!dst) continue;
        for (int r = wave; r < kTM; r += kTN / 64) {
            const int row = r0 + r;
            if (row >= M) break;
            float* orow = dst + img_off + (size_t)row * ld;
            const int cc = c0 + 4 * lane;
            const float4 v = *reinterpret_cast<const float4*>(&s.out[o][r][4 * lane]);
            if (vec && cc + 3 < N) {
                gnms_iou::store_nt_f4(orow + cc, v.x, v.y, v.z, v.w);
            } else {
                if (cc < N) orow[cc] = v.x;
                if (cc + 1 < N) orow[cc + 1] = v.y;
                if (cc + 2 < N) orow[cc + 2] = v.z;
                if (cc + 3 < N) orow[cc + 3] = v.w;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// float64 list: pair i = (corners_a[i], corners_b[i]), one thread per pair (the drop-in's sizes: a few hundred pairs).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iou3d_exact_list_f64_kernel(const double* __restrict__ A, const double* __restrict__ Bx, long count,
                                                                   const double* __restrict__ vol, double* __restrict__ bev,
                                                                   double* __restrict__ i3) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Rec<double> ra, rb;
    {
        double cx[8], cy[8], cz[8];
        const double* p = A + i * 24;
#pragma unroll
        for (int k = 0; k < 8; ++k) { cx[k] = p[k]; cy[k] = p[8 + k]; cz[k] = p[16 + k]; }
        make_rec(cx, cy, cz, 1, ra);
        p = Bx + i * 24;
#pragma unroll
        for (int k = 0; k < 8; ++k) { cx[k] = p[k]; cy[k] = p[8 + k]; cz[k] = p[16 + k]; }
        make_rec(cx, cy, cz, 1, rb);
    }
    const double yov = fmax(0.0, fmin(ra.y1, rb.y1) - fmax(ra.y0, rb.y0));                     // :286
    double I = 0.0;
    const bool xz = fmax(ra.x0, rb.x0) < fmin(ra.x1, rb.x1) && fmax(ra.z0, rb.z0) < fmin(ra.z1, rb.z1);
    if (xz && ra.area > 0.0 && rb.area > 0.0) {
        const double ox = ra.vx[0], oz = ra.vz[0];
        double ax[4], az[4], bx[4], bz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ax[q] = ra.vx[q] - ox; az[q] = ra.vz[q] - oz; bx[q] = rb.vx[q] - ox; bz[q] = rb.vz[q] - oz; }
        I = intersection_area(ax, az, bx, bz);
    }
    const double v = vol ? vol[i] : ra.vol + rb.vol;                                             // :276-277
    const double I3 = yov * I;
    if (bev) bev[i] = I / ((rb.area + ra.area) - I);
    if (i3) i3[i] = I3 / (v - I3);
}

int iou3d_exact_common(const float* a, const float* b, bool from_params, int B, int M, int N, int volume_mode, float* bev, float* i3,
                       int64_t ld, void* stream, const char* name) {
    GNMS_CHECK_ARG(B >= 0 && M >= 0 && N >= 0, "%s: negative size (B=%d M=%d N=%d)", name, B, M, N);
    GNMS_CHECK_ARG(volume_mode == 0 || volume_mode == 1, "%s: volume_mode %d not in {0,1}", name, volume_mode);
    if (B == 0 || M == 0 || N == 0) return GNMS_OK;
    GNMS_CHECK_ARG(a && b, "%s: null input", name);
    GNMS_CHECK_ARG(bev || i3, "%s: iou_bev and iou_3d are both NULL", name);
    GNMS_CHECK_ARG(ld >= N, "%s: ld (%lld) < N (%d)", name, (long long)ld, N);
    GNMS_CHECK_ARG(gnms_div_up(M, kTM) <= 65535 && B <= 65535, "%s: M / %d and B must be <= 65535", name, kTM);
    const int vec = (ld % 4 == 0) && (!bev || (uintptr_t)bev % 16 == 0) && (!i3 || (uintptr_t)i3 % 16 == 0);
    const dim3 grid(gnms_div_up(N, kTN), gnms_div_up(M, kTM), B);
    hipStream_t st = (hipStream_t)stream;
    if (from_params) iou3d_exact_kernel<true><<<grid, kTN, 0, st>>>(a, b, M, N, volume_mode, bev, i3, (long)ld, vec);
    else iou3d_exact_kernel<false><<<grid, kTN, 0, st>>>(a, b, M, N, volume_mode, bev, i3, (long)ld, vec);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

}  // namespace

extern "C" int gnms_iou3d_exact(const float* corners_a, const float* corners_b, int B, int M, int N, int volume_mode, float* iou_bev,
                                float* iou_3d, int64_t ld, void* stream) {
    return iou3d_exact_common(corners_a, corners_b, false, B, M, N, volume_mode, iou_bev, iou_3d, ld, stream, "gnms_iou3d_exact");
}

extern "C" int gnms_iou3d_exact_from_params(const float* params_a, const float* params_b, int B, int M, int N, int volume_mode,
                                            float* iou_bev, float* iou_3d, int64_t ld, void* stream) {
    return iou3d_exact_common(params_a, params_b, true, B, M, N, volume_mode, iou_bev, iou_3d, ld, stream, "gnms_iou3d_exact_from_params");
}

extern "C" int gnms_iou3d_exact_list_f64(const double* corners_a, const double* corners_b, int64_t count, const double* vol, double* iou_bev,
                                         double* iou_3d, void* stream) {
    GNMS_CHECK_ARG(count >= 0, "gnms_iou3d_exact_list_f64: negative count");
    if (count == 0) return GNMS_OK;
    GNMS_CHECK_ARG(corners_a && corners_b, "gnms_iou3d_exact_list_f64: null input");
    GNMS_CHECK_ARG(iou_bev || iou_3d, "gnms_iou3d_exact_list_f64: iou_bev and iou_3d are both NULL");
    iou3d_exact_list_f64_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(corners_a, corners_b, (long)count, vol,
                                                                                                  iou_bev, iou_3d);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
