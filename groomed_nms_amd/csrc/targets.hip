// targets.hip -- anchor training targets (the reference's compute_targets, lib/rpn_util.py:411-524, and iou_ign, lib/core.py:535-575)
// on the device, for B images at once.
//
// Two stream-ordered launches, no atomics, no inter-workgroup waits, no allocation:
//   targets_tile   one lane per roi: ols_ign_max, ols[r, :], ols_max, target = first argmax; the roi's whole output row (fg when
//                  ols_max >= fg, else bg / all-zero), staged in LDS and written as one contiguous span per tile.  Each workgroup
//                  covers TGT_TILES_PER_WG consecutive tiles and leaves, per GT, the maximum of ols[:, j] over its rois (as ordered
//                  bits) and the first roi attaining it in the caller's workspace: plain stores, one slot per (image, workgroup, GT)
//   targets_best   one wave per (image, GT): the first maximum over the workgroups' slots (they are in roi order), best_roi[b][j],
//                  and the kept best roi's row rewritten as fg (idempotent: two GTs that share a roi write the same row, because the
//                  row depends on the roi's own target only)
//
// Precision is NumPy's type promotion (lib/rpn_util.py with float64 ground truths): what depends on the roi alone (area, widths,
// centres) is computed in the rois' type T, everything that touches a GT in float64, and each value is rounded once into the
// float32 outputs.  NaN follows np.amax / np.argmax (NaN is the maximum, the first NaN wins) and every comparison with NaN is false.
#include <math.h>
#include "gnms_common.h"

namespace {

constexpr int TGT_THREADS = 128;      // rois per tile (staging: 128 rows of <= 32 + 29 floats)
constexpr int TGT_TILES_PER_WG = 2;   // consecutive tiles per workgroup of targets_tile
constexpr int TGT_WAVES = TGT_THREADS / GNMS_WAVE;

struct TgtArgs {
    const void* rois;
    long long ld_rois;
    int B, R, M, K, D3, has_3d;
    const double* gts_val;
    const int32_t* lbls;
    const int32_t* val_counts;
    const double* gts_ign;
    const int32_t* ign_counts;
    const double* gts_3d;
    const void* rois_3d;
    long long ld_rois_3d;
    int rois_3d_f64;
    const void* cen;
    int cen_f64;
    const double* anchors;
    int A, anchor_cols, tracker_col;
    int decomp, vel, n_src3d;   // n_src3d: columns of src_3d = rois_3d[:, 4:] / anchors[tracker, 4:] that are read
    int Wt, Wr, n_norm3;        // output widths; columns 5 .. 5 + n_norm3 - 1 are normalised with means[4 ..]
    int use_means, use_stds;
    double fg, ign, bg_lo, bg_hi, best;
    double means[13], stds[13];
    float* transforms;
    float* raw_gt;
    double* ols_max;
    double* ols;
    double* ols_ign;
    long long* best_roi;
    int nwg;                      // workgroups per image of targets_tile
    unsigned long long* keys;     // [B][nwg][M] ordered bits of the workgroup's max_r ols[r, j]
    unsigned int* firsts;         // [B][nwg][M] the first of its rois attaining it
};

// np.minimum / np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }
// np.clip(d, 0, None): NaN stays NaN
__device__ __forceinline__ double clip0(double d) { return d < 0.0 ? 0.0 : d; }

// lib/core.py:205-218 (intersect, combinations, ndarray): box_a the roi (widened), box_b the GT
__device__ __forceinline__ double inter_of(double x1, double y1, double x2, double y2, const double* g) {
    const double iw = clip0(np_min(x2, g[2]) - np_max(x1, g[0]));
    const double ih = clip0(np_min(y2, g[3]) - np_max(y1, g[1]));
    return iw * ih;
}

// x / u as IEEE division gives it, without the division when x is a zero and u a nonzero number (most pairs do not overlap)
__device__ __forceinline__ double div0(double x, double u) {
    if (x == 0.0 && fabs(u) > 0.0) return (signbit(x) != signbit(u)) ? -0.0 : 0.0;
    return x / u;
}

// a total order of doubles as uint64 that np.amax agrees with: -0 == +0, every NaN above +inf
__device__ __forceinline__ unsigned long long okey(double v) {
    if (v != v) return ~0ull;
    if (v == 0.0) v = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double okey_value(unsigned long long k) {
    if (k == ~0ull) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// np.amax / np.argmax over a row: NaN is the maximum and the first NaN (or the first maximum) wins
__device__ __forceinline__ void argmax_step(double o, int j, double& m, int& arg) {
    if (j == 0 || (m == m && (o != o || o > m))) { m = o; arg = j; }
}

template <typename T>
__device__ __forceinline__ T ld_t(const void* p, long long i) { return static_cast<const T*>(p)[i]; }
__device__ __forceinline__ double ld_any(const void* p, int f64, long long i) {
    return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

__device__ __forceinline__ int clamp_count(const int32_t* counts, int b, int cap) {
    if (!counts) return cap;
    const int c = counts[b];
    return c < 0 ? 0 : (c > cap ? cap : c);
}

// the call site's in-place normalisation (lib/loss/rpn_3d.py:440-451): float32 -= float64, float32 /= float64, each step in float64
// and rounded to float32.  nm = LDS [means 13 | stds 13].
__device__ __forceinline__ float tcol(const TgtArgs& a, const double* nm, int c, double v) {
    float f = (float)v;
    const int mi = c < 4 ? c : ((c >= 5 && c < 5 + a.n_norm3) ? c - 1 : -1);
    if (mi >= 0) {
        if (a.use_means) f = (float)((double)f - nm[mi]);
        if (a.use_stds) f = (float)((double)f / nm[13 + mi]);
    }
    return f;
}

// One output row: kind 2 = fg (target j), 1 = bg (label -1), 0 = all zero (label 0: ignore).  t / g are the row's first elements
// (LDS staging or global memory); either may be null.
template <typename T>
__device__ void emit_row(const TgtArgs& a, const double* nm, int b, int r, int kind, int j, T x1, T y1, T x2, T y2, float* t, float* g) {
    if (kind != 2) {
        if (t)
            for (int c = 0; c < a.Wt; ++c) t[c] = c == 4 ? (kind == 1 ? -1.0f : 0.0f) : tcol(a, nm, c, 0.0);
        if (g)
            for (int c = 0; c < a.Wr; ++c) g[c] = 0.0f;
        return;
    }
    const double* gv = a.gts_val + ((long long)b * a.M + j) * 4;
    const double* g3 = a.has_3d ? a.gts_3d + ((long long)b * a.M + j) * a.D3 : nullptr;
    // lib/rpn_util.py:843-869 bbox_transform: the roi's widths and centres in T (float32 rois: NEP 50 keeps the Python scalars weak)
    const T ew = x2 - x1 + (T)1.0;
    const T eh = y2 - y1 + (T)1.0;
    const T ecx = x1 + (T)0.5 * ew;
    const T ecy = y1 + (T)0.5 * eh;
    if (t) {
        const double gw = gv[2] - gv[0] + 1.0;
        const double gh = gv[3] - gv[1] + 1.0;
        const double gcx = gv[0] + 0.5 * gw;
        const double gcy = gv[1] + 0.5 * gh;
        t[0] = tcol(a, nm, 0, (gcx - (double)ecx) / (double)ew);
        t[1] = tcol(a, nm, 1, (gcy - (double)ecy) / (double)eh);
        t[2] = tcol(a, nm, 2, log(gw / (double)ew));
        t[3] = tcol(a, nm, 3, log(gh / (double)eh));
        t[4] = (float)a.lbls[(long long)b * a.M + j];
        if (a.has_3d) {
            // src_3d = rois_3d[r, 4:] or anchors[int64(tracker[r]), 4:] (:474-477)
            double s[8];
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            if (a.rois_3d) {
                const long long base = ((long long)b * a.R + r) * a.ld_rois_3d + 4;
#pragma unroll
                for (int c = 0; c < 8; ++c) s[c] = c < a.n_src3d ? ld_any(a.rois_3d, a.rois_3d_f64, base + c) : 0.0;
            } else {
                const T tv = ld_t<T>(a.rois, ((long long)b * a.R + r) * a.ld_rois + a.tracker_col);
                long long ti = (tv > (T)-9.0e18 && tv < (T)9.0e18) ? (long long)tv : (long long)1 << 62;   // astype(int64): truncation
                if (ti < 0) ti += a.A;                                                                         // NumPy's negative index
                const bool ok = ti >= 0 && ti < a.A;
#pragma unroll
                for (int c = 0; c < 8; ++c) s[c] = c < a.n_src3d ? (ok ? a.anchors[ti * a.anchor_cols + 4 + c] : qnan) : 0.0;
            }
            // lib/rpn_util.py:794-840 bbox_transform_3d
            const double cx = a.cen ? ld_any(a.cen, a.cen_f64, ((long long)b * a.R + r) * 2 + 0) : (double)ecx;
            const double cy = a.cen ? ld_any(a.cen, a.cen_f64, ((long long)b * a.R + r) * 2 + 1) : (double)ecy;
            int c = 5;
            t[c] = tcol(a, nm, c, (g3[0] - cx) / (double)ew); ++c;
            t[c] = tcol(a, nm, c, (g3[1] - cy) / (double)eh); ++c;
            t[c] = tcol(a, nm, c, g3[2] - s[0]); ++c;
            t[c] = tcol(a, nm, c, log(g3[3] / s[1])); ++c;
            t[c] = tcol(a, nm, c, log(g3[4] / s[2])); ++c;
            t[c] = tcol(a, nm, c, log(g3[5] / s[3])); ++c;
            t[c] = tcol(a, nm, c, g3[6] - s[4]); ++c;
            if (a.decomp) {
                t[c] = tcol(a, nm, c, g3[12] - s[5]); ++c;
                t[c] = tcol(a, nm, c, g3[13] - s[6]); ++c;
                if (a.vel) { t[c] = tcol(a, nm, c, a.D3 == 17 ? g3[16] - s[7] : -INFINITY); ++c; }
            }
            for (int k = 7; k < a.D3; ++k, ++c) t[c] = tcol(a, nm, c, g3[k]);   // np.hstack((targets, gt_rois[:, 7:]))
        }
    }
    if (g) {
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = (float)gv[c];
        g[4] = 0.0f;                                                             // raw_gt[:, 4] is never written (:475)
        if (a.has_3d)
            for (int k = 0; k < a.D3; ++k) g[5 + k] = (float)g3[k];
    }
}

// LDS layout shared by the three kernels: [gts 4M | area M | ign 4K | area_ign * 0 K | means 13 | stds 13] doubles, then the staging
__device__ int load_gts(const TgtArgs& a, int b, double* sm, int& Mb, int& Kb) {
    Mb = clamp_count(a.val_counts, b, a.M);
    Kb = clamp_count(a.ign_counts, b, a.K);
    double* gv = sm;
    double* av = gv + 4 * a.M;
    double* gi = av + a.M;
    double* zi = gi + 4 * a.K;
    double* nm = zi + a.K;
    for (int i = threadIdx.x; i < 4 * Mb; i += blockDim.x) gv[i] = a.gts_val[(long long)b * a.M * 4 + i];
    for (int i = threadIdx.x; i < 4 * Kb; i += blockDim.x) gi[i] = a.gts_ign[(long long)b * a.K * 4 + i];
    for (int i = threadIdx.x; i < 26; i += blockDim.x) nm[i] = i < 13 ? a.means[i] : a.stds[i - 13];
    __syncthreads();
    for (int j = threadIdx.x; j < Mb; j += blockDim.x) av[j] = (gv[4 * j + 2] - gv[4 * j]) * (gv[4 * j + 3] - gv[4 * j + 1]);
    for (int k = threadIdx.x; k < Kb; k += blockDim.x) zi[k] = ((gi[4 * k + 2] - gi[4 * k]) * (gi[4 * k + 3] - gi[4 * k + 1])) * 0.0;
    __syncthreads();
    return 0;
}

template <typename T>
__device__ __forceinline__ void load_roi(const TgtArgs& a, int b, int r, T& x1, T& y1, T& x2, T& y2) {
    const long long base = ((long long)b * a.R + r) * a.ld_rois;
    x1 = ld_t<T>(a.rois, base);
    y1 = ld_t<T>(a.rois, base + 1);
    x2 = ld_t<T>(a.rois, base + 2);
    y2 = ld_t<T>(a.rois, base + 3);
}

// lib/core.py:510-519: inter / (area_a + area_b - inter), area_a in T then widened
__device__ __forceinline__ double iou_of(double x1, double y1, double x2, double y2, double area_a, const double* gv, const double* av, int j) {
    const double in = inter_of(x1, y1, x2, y2, gv + 4 * j);
    return div0(in, (area_a + av[j]) - in);
}

template <typename T>
__global__ __launch_bounds__(TGT_THREADS) void targets_tile(TgtArgs a) {
    extern __shared__ double sm[];
    const int b = blockIdx.y;
    int Mb, Kb;
    load_gts(a, b, sm, Mb, Kb);
    const double* gv = sm;
    const double* av = gv + 4 * a.M;
    const double* gi = av + a.M;
    const double* zi = gi + 4 * a.K;
    const double* nm = zi + a.K;
    // per GT: the workgroup's running maximum (bk, br) and each wave's of the current tile (wk, wr)
    unsigned long long* bk = reinterpret_cast<unsigned long long*>(const_cast<double*>(nm) + 26);
    unsigned long long* wk = bk + a.M;
    unsigned int* br = reinterpret_cast<unsigned int*>(wk + TGT_WAVES * a.M);
    unsigned int* wr = br + a.M;
    float* st_t = reinterpret_cast<float*>(wr + TGT_WAVES * a.M + (a.M & 1));
    float* st_g = st_t + TGT_THREADS * a.Wt;
    for (int j = threadIdx.x; j < Mb; j += TGT_THREADS) bk[j] = 0ull;      // below every real key (dead lanes carry 0 too)
    const int lane = threadIdx.x & (GNMS_WAVE - 1);
    const int wave = threadIdx.x / GNMS_WAVE;

    for (int tile = 0; tile < TGT_TILES_PER_WG; ++tile) {
        const int r0 = (blockIdx.x * TGT_TILES_PER_WG + tile) * TGT_THREADS;
        if (r0 >= a.R) break;                                            // uniform
        const int r = r0 + threadIdx.x;
        const bool live = r < a.R;
        T x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (live) load_roi<T>(a, b, r, x1, y1, x2, y2);
        const T area_t = (x2 - x1) * (y2 - y1);
        const double area_a = (double)area_t;
        const double dx1 = x1, dy1 = y1, dx2 = x2, dy2 = y2;
        const long long row = (long long)b * a.R + r;

        // iou_ign (lib/core.py:535-575): inter / (area_a + area_b * 0 - inter * 0); its row maximum (0 without ignore boxes)
        double im = 0.0;
        int dummy = 0;
        for (int k = 0; k < Kb; ++k) {
            const double in = inter_of(dx1, dy1, dx2, dy2, gi + 4 * k);
            const double o = div0(in, (area_a + zi[k]) - in * 0.0);
            if (live && a.ols_ign) a.ols_ign[row * a.K + k] = o;
            argmax_step(o, k, im, dummy);
        }
        if (live && a.ols_ign)
            for (int k = Kb; k < a.K; ++k) a.ols_ign[row * a.K + k] = 0.0;

        double om = 0.0;
        int tg = 0;
        for (int j = 0; j < Mb; ++j) {
            const double o = iou_of(dx1, dy1, dx2, dy2, area_a, gv, av, j);
            if (live && a.ols) a.ols[row * a.M + j] = o;
            argmax_step(o, j, om, tg);
            const unsigned long long key = live ? okey(o) : 0ull;
            // the wave's maximum and its first roi.  Most waves do not touch a given GT: when no lane is above +0 and one is at +0,
            // that is the answer without the cross-lane reduction (a chain of 12 LDS permutes)
            unsigned long long k = 1ull << 63;                          // okey(+0.0)
            unsigned long long hit = __ballot(key == k);
            if (__ballot(key > k) != 0 || hit == 0) {                   // uniform
                k = key;
#pragma unroll
                for (int s = 1; s < GNMS_WAVE; s <<= 1) {
                    const unsigned long long q = __shfl_xor(k, s);
                    k = q > k ? q : k;
                }
                hit = __ballot(key == k);
            }
            if (lane == 0) {
                wk[wave * a.M + j] = k;
                wr[wave * a.M + j] = (unsigned int)(r0 + wave * GNMS_WAVE + __ffsll((long long)hit) - 1);
            }
        }
        if (live && a.ols)
            for (int j = Mb; j < a.M; ++j) a.ols[row * a.M + j] = 0.0;
        if (live && a.ols_max) a.ols_max[row] = om;

        // lib/rpn_util.py:448-516: fg = ols_max >= fg (the kept best rois follow in targets_best), bg = lo <= ols_max < hi minus ign
        int kind;
        if (Mb == 0 && Kb == 0) kind = 1;                               // :518-521 all background
        else if (Mb > 0 && om >= a.fg) kind = 2;
        else kind = (om >= a.bg_lo && om < a.bg_hi && !(im >= a.ign)) ? 1 : 0;
        if (live)
            emit_row<T>(a, nm, b, r, kind, tg, x1, y1, x2, y2, a.transforms ? st_t + threadIdx.x * a.Wt : nullptr,
                        a.raw_gt ? st_g + threadIdx.x * a.Wr : nullptr);
        __syncthreads();
        for (int j = threadIdx.x; j < Mb; j += TGT_THREADS)              // waves in roi order, strict >: the first maximum stays
            for (int w = 0; w < TGT_WAVES; ++w)
                if (wk[w * a.M + j] > bk[j]) { bk[j] = wk[w * a.M + j]; br[j] = wr[w * a.M + j]; }
        const int nrows = min(TGT_THREADS, a.R - r0);
        const long long first = (long long)b * a.R + r0;
        if (a.transforms)
            for (int i = threadIdx.x; i < nrows * a.Wt; i += TGT_THREADS) a.transforms[first * a.Wt + i] = st_t[i];
        if (a.raw_gt)
            for (int i = threadIdx.x; i < nrows * a.Wr; i += TGT_THREADS) a.raw_gt[first * a.Wr + i] = st_g[i];
        __syncthreads();
    }
    const long long slot = ((long long)b * a.nwg + blockIdx.x) * a.M;
    for (int j = threadIdx.x; j < Mb; j += TGT_THREADS) {
        a.keys[slot + j] = bk[j];
        a.firsts[slot + j] = br[j];
    }
}

// one wave per (image, GT): the first roi attaining max_r ols[r, j] (lib/rpn_util.py:456-460), kept when it passes best_thresh;
// best_roi, and the kept roi's row as fg with the roi's own target (:462-503)
template <typename T>
__global__ __launch_bounds__(GNMS_WAVE) void targets_best(TgtArgs a) {
    extern __shared__ double sm[];
    const int j = blockIdx.x, b = blockIdx.y;
    int Mb, Kb;
    load_gts(a, b, sm, Mb, Kb);
    const double* gv = sm;
    const double* av = gv + 4 * a.M;
    const double* nm = av + a.M + 5 * a.K;
    long long out = -1;
    if (j < Mb && a.R > 0) {
        // lane l scans workgroups l, l + 64, ... (in roi order: strict > keeps the first), then the wave: max key, lowest roi
        unsigned long long k = 0ull;
        unsigned int r = 0xffffffffu;
        for (int w = threadIdx.x; w < a.nwg; w += GNMS_WAVE) {
            const long long slot = ((long long)b * a.nwg + w) * a.M + j;
            const unsigned long long q = a.keys[slot];
            if (q > k) { k = q; r = a.firsts[slot]; }
        }
        unsigned long long km = k;
#pragma unroll
        for (int s = 1; s < GNMS_WAVE; s <<= 1) {
            const unsigned long long q = __shfl_xor(km, s);
            km = q > km ? q : km;
        }
        unsigned int rm = k == km ? r : 0xffffffffu;
#pragma unroll
        for (int s = 1; s < GNMS_WAVE; s <<= 1) {
            const unsigned int q = __shfl_xor(rm, s);
            rm = q < rm ? q : rm;
        }
        if (okey_value(km) >= a.best && rm < (unsigned int)a.R) {
            out = rm;
            if (threadIdx.x == 0) {
                const int rr = (int)rm;
                T x1, y1, x2, y2;
                load_roi<T>(a, b, rr, x1, y1, x2, y2);
                const double area_a = (double)((x2 - x1) * (y2 - y1));
                double om = 0.0;
                int tg = 0;
                for (int i = 0; i < Mb; ++i) argmax_step(iou_of(x1, y1, x2, y2, area_a, gv, av, i), i, om, tg);
                const long long row = (long long)b * a.R + rr;
                emit_row<T>(a, nm, b, rr, 2, tg, x1, y1, x2, y2, a.transforms ? a.transforms + row * a.Wt : nullptr,
                            a.raw_gt ? a.raw_gt + row * a.Wr : nullptr);
            }
        }
    }
    if (threadIdx.x == 0 && a.best_roi) a.best_roi[(long long)b * a.M + j] = out;
}

size_t gts_lds_bytes(int M, int K) { return sizeof(double) * (5 * (size_t)M + 5 * (size_t)K + 26); }

int nwg_of(int R) { return (R + TGT_THREADS * TGT_TILES_PER_WG - 1) / (TGT_THREADS * TGT_TILES_PER_WG); }

template <typename T>
int launch(const TgtArgs& a, hipStream_t st) {
    const size_t lds_g = gts_lds_bytes(a.M, a.K);
    if (a.R > 0) {
        const size_t lds_tile = lds_g + (sizeof(unsigned long long) + sizeof(unsigned int)) * (TGT_WAVES + 1) * (size_t)a.M + 4 +
                                sizeof(float) * TGT_THREADS * (a.Wt + a.Wr);
        targets_tile<T><<<dim3(a.nwg, a.B), TGT_THREADS, lds_tile, st>>>(a);
        GNMS_CHECK_LAUNCH();
    }
    if (a.M > 0) {
        targets_best<T><<<dim3(a.M, a.B), GNMS_WAVE, lds_g, st>>>(a);
        GNMS_CHECK_LAUNCH();
    }
    return GNMS_OK;
}

}  // namespace

extern "C" size_t gnms_compute_targets_workspace_bytes(int B, int R, int M) {
    if (B <= 0 || R <= 0 || M <= 0) return 0;
    return (size_t)B * (size_t)nwg_of(R) * (size_t)M * (sizeof(unsigned long long) + sizeof(unsigned int));
}

extern "C" int gnms_compute_targets(const void* rois, int rois_f64, int B, int R, int64_t ld_rois, const double* gts_val,
                                    const int32_t* box_lbls, int M, const int32_t* val_counts, const double* gts_ign, int K,
                                    const int32_t* ign_counts, const double* gts_3d, int D3, const void* rois_3d, int rois_3d_f64,
                                    int64_t ld_rois_3d, const void* rois_3d_cen, int cen_f64, const double* anchors, int A, int anchor_cols,
                                    int tracker_col, double fg_thresh, double ign_thresh, double bg_thresh_lo, double bg_thresh_hi,
                                    double best_thresh, const double* means_host, const double* stds_host, float* transforms,
                                    float* raw_gt, double* ols_max, double* ols, double* ols_ign, int64_t* best_roi, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && R >= 0 && M >= 0 && K >= 0, "gnms_compute_targets: negative size");
    if (M > GNMS_TARGETS_MAX_GTS || K > GNMS_TARGETS_MAX_GTS) {
        gnms_set_error("gnms_compute_targets: %d ground truths / %d ignore boxes per image, at most %d", M, K, GNMS_TARGETS_MAX_GTS);
        return GNMS_ERR_UNSUPPORTED;
    }
    GNMS_CHECK_ARG(B <= 65535, "gnms_compute_targets: B = %d > 65535", B);
    GNMS_CHECK_ARG((long long)R * B < (1ll << 40) && R < (1 << 30), "gnms_compute_targets: R = %d too large", R);
    GNMS_CHECK_ARG(anchor_cols == 0 || anchor_cols >= 4, "gnms_compute_targets: anchor_cols = %d", anchor_cols);
    const int decomp = anchor_cols >= 11, vel = anchor_cols == 12;                       // lib/rpn_util.py:420-421
    // D3 alone says whether the targets are 3D (and so sets the output widths): gts_3d may be NULL when no image has a GT row
    GNMS_CHECK_ARG(D3 >= 0, "gnms_compute_targets: D3 = %d", D3);
    const int has_3d = D3 != 0;
    if (has_3d) {
        GNMS_CHECK_ARG(D3 >= 7 && D3 <= GNMS_TARGETS_MAX_D3, "gnms_compute_targets: D3 = %d outside [7, %d]", D3, GNMS_TARGETS_MAX_D3);
        GNMS_CHECK_ARG(!decomp || D3 >= 14, "gnms_compute_targets: decomp_alpha reads gts_3d[:, 12:14], D3 = %d", D3);
    }
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(R == 0 || rois, "gnms_compute_targets: rois is NULL");
    GNMS_CHECK_ARG(ld_rois >= 4, "gnms_compute_targets: ld_rois = %lld < 4", (long long)ld_rois);
    GNMS_CHECK_ARG(M == 0 || (gts_val && box_lbls), "gnms_compute_targets: gts_val / box_lbls is NULL");
    GNMS_CHECK_ARG(K == 0 || gts_ign, "gnms_compute_targets: gts_ign is NULL");
    GNMS_CHECK_ARG(M == 0 || !has_3d || gts_3d, "gnms_compute_targets: D3 = %d and gts_3d is NULL", D3);
    const int n_src3d = decomp ? (vel && D3 == 17 ? 8 : 7) : 5;
    if (has_3d && M > 0 && R > 0) {
        if (rois_3d) {
            GNMS_CHECK_ARG(ld_rois_3d >= 4 + n_src3d, "gnms_compute_targets: ld_rois_3d = %lld, rois_3d[:, 4:] needs %d columns",
                           (long long)ld_rois_3d, n_src3d);
        } else {
            GNMS_CHECK_ARG(anchors && A > 0, "gnms_compute_targets: neither rois_3d nor anchors");
            GNMS_CHECK_ARG(anchor_cols >= 4 + n_src3d, "gnms_compute_targets: anchor_cols = %d, anchors[:, 4:] needs %d columns", anchor_cols,
                           n_src3d);
            GNMS_CHECK_ARG(tracker_col >= 0 && tracker_col < ld_rois, "gnms_compute_targets: tracker_col = %d outside the rois' row of %lld",
                           tracker_col, (long long)ld_rois);
        }
    }
    const size_t need = gnms_compute_targets_workspace_bytes(B, R, M);
    if (need) {
        if (!workspace || workspace_bytes < need) {
            gnms_set_error("gnms_compute_targets: workspace of %zu bytes, needs %zu", workspace_bytes, need);
            return GNMS_ERR_WORKSPACE;
        }
        GNMS_CHECK_ARG((uintptr_t)workspace % 8 == 0, "gnms_compute_targets: workspace must be 8-byte aligned");
    }

    TgtArgs a = {};
    a.rois = rois;
    a.ld_rois = ld_rois;
    a.B = B; a.R = R; a.M = M; a.K = K;
    a.has_3d = has_3d;
    a.D3 = has_3d ? D3 : 0;
    a.gts_val = gts_val; a.lbls = box_lbls; a.val_counts = val_counts;
    a.gts_ign = gts_ign; a.ign_counts = ign_counts;
    a.gts_3d = gts_3d;
    a.rois_3d = rois_3d; a.ld_rois_3d = ld_rois_3d; a.rois_3d_f64 = rois_3d_f64 != 0;
    a.cen = rois_3d_cen; a.cen_f64 = cen_f64 != 0;
    a.anchors = anchors; a.A = A; a.anchor_cols = anchor_cols; a.tracker_col = tracker_col;
    a.decomp = decomp; a.vel = vel; a.n_src3d = n_src3d;
    a.Wt = has_3d ? 5 + D3 + 2 * decomp + vel : 5;
    a.Wr = has_3d ? 5 + D3 : 5;
    a.n_norm3 = has_3d ? (decomp ? 9 : 7) : 0;
    a.use_means = means_host != nullptr;
    a.use_stds = stds_host != nullptr;
    for (int i = 0; i < 4 + a.n_norm3; ++i) {
        a.means[i] = means_host ? means_host[i] : 0.0;
        a.stds[i] = stds_host ? stds_host[i] : 1.0;
    }
    a.fg = fg_thresh; a.ign = ign_thresh; a.bg_lo = bg_thresh_lo; a.bg_hi = bg_thresh_hi; a.best = best_thresh;
    a.transforms = transforms; a.raw_gt = raw_gt; a.ols_max = ols_max; a.ols = ols; a.ols_ign = ols_ign;
    a.best_roi = (long long*)best_roi;
    a.nwg = nwg_of(R);
    a.keys = static_cast<unsigned long long*>(workspace);
    a.firsts = a.keys ? reinterpret_cast<unsigned int*>(a.keys + (size_t)B * a.nwg * M) : nullptr;

    hipStream_t st = (hipStream_t)stream;
    return rois_f64 ? launch<double>(a, st) : launch<float>(a, st);
}
