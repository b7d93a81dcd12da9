// kitti_eval.hip -- the KITTI object evaluation (data/kitti_split1/devkit/cpp/evaluate_object*.cpp) for gfx950 (MI355X): 2D AP, AOS,
// bird's-eye-view AP and 3D AP of every class and difficulty, for any number of (MIN_OVERLAP table, ground-truth distance cut)
// variants in one call.  The devkit is the specification, decision for decision; line numbers below are evaluate_object.cpp's.
//
// Data: det [n_det][14] and gt [n_gt][15] float64 rows (GNMS_KITTI_DET_* / GNMS_KITTI_GT_* columns), ragged over images by
// det_offsets / gt_offsets [I + 1]; pair_offsets [I + 1] = running sum of (detections x ground truths) per image.
//
//   flags      one thread per detection: compute_aos and the eval_image / eval_ground / eval_3d switches (:175-186), integer atomics.
//   overlaps   one workgroup per image, one thread per (ground truth, detection) pair: imageBoxOverlap, groundBoxOverlap and
//              box3DOverlap (:247-364) with criterion -1, and with criterion 0 (over the detection's own area / volume) on DontCare rows
//              -- the only value the devkit ever reads for them (:600; their ignored_gt is -1 for every class).  The criterion is an
//              argument of the one overlap function.  ov[metric][pair_offsets[img] + g * nd + j].  Footprints are toPolygon's (:289-311);
//              boost's intersection is the clip of bev_clip.h, its union area is area_d + area_g - I.  Computed once, read by all variants.
//   recall     computeStatistics with compute_fp = false (:476-573): one LANE per (image, class, metric, difficulty, variant); the score
//              of the true positive of ground-truth row g goes to slot g of the curve's score row, -inf where there is none.
//   (the caller sorts each score row in descending order)
//   thresholds getThresholds' scan (:366-399), one lane per curve.
//   precision  computeStatistics with compute_fp = true (:476-633): one wave per (image, curve), lane t = threshold t.  tp / fp / fn are
//              integer atomics; the similarity goes to a per-image buffer.
//   finish     per curve: similarity summed in image order (deterministic; no floating-point atomics anywhere), precision and aos,
//              max_{i..end} (:700-719).
// Both passes run the one device function below; each lane keeps its own assigned_detection bit set in a column of LDS
// (GNMS_KITTI_EVAL_MAX_DET bits).  Every loop bound is a count from the offsets; no lane waits for another.
#include "gnms_common.h"
#include "bev_clip.h"

namespace {

using namespace gnms_bev;

constexpr int kDetCols = 14, kGtCols = 15;
constexpr int kCurves = GNMS_KITTI_EVAL_CURVES;        // class * 9 + metric * 3 + difficulty
constexpr int kPts = GNMS_KITTI_EVAL_PTS;              // N_SAMPLE_PTS (:64)
constexpr int kMaxDet = GNMS_KITTI_EVAL_MAX_DET;
constexpr int kWords = kMaxDet / 64;
// flags[]: [0] = some detection has alpha == -10 (compute_aos = false), [1 + c] eval_image, [4 + c] eval_ground, [7 + c] eval_3d
constexpr int kFlags = 10;

enum { T_CAR = 0, T_PED = 1, T_CYC = 2, T_VAN = 3, T_SIT = 4, T_DC = 5 };       // type ids (anything else: "other")

__device__ __forceinline__ int min_height(int d) { return d == 0 ? 40 : 25; }                    // MIN_HEIGHT (:49)
__device__ __forceinline__ int max_occlusion(int d) { return d; }                                // MAX_OCCLUSION (:50)
__device__ __forceinline__ double max_truncation(int d) { return d == 0 ? 0.15 : (d == 1 ? 0.3 : 0.5); }   // MAX_TRUNCATION (:51)

__global__ __launch_bounds__(256) void flags_kernel(const double* __restrict__ det, int n_det, int* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_det) return;
    const double* d = det + (size_t)i * kDetCols;
    if (d[GNMS_KITTI_DET_ALPHA] == -10.0) atomicOr(&flags[0], 1);                                // :175
    const int c = (int)d[GNMS_KITTI_DET_CLASS];
    if (!(d[GNMS_KITTI_DET_CLASS] >= 0.0 && d[GNMS_KITTI_DET_CLASS] <= 2.0)) return;             // :180
    const double h = d[GNMS_KITTI_DET_H], w = d[GNMS_KITTI_DET_H + 1], l = d[GNMS_KITTI_DET_H + 2];
    const double t1 = d[GNMS_KITTI_DET_T], t2 = d[GNMS_KITTI_DET_T + 1], t3 = d[GNMS_KITTI_DET_T + 2];
    if (d[GNMS_KITTI_DET_X1] >= 0.0) atomicOr(&flags[1 + c], 1);                                 // :181
    if (t1 != -1000.0 && t3 != -1000.0 && w > 0.0 && l > 0.0) atomicOr(&flags[4 + c], 1);        // :183
    if (t1 != -1000.0 && t2 != -1000.0 && t3 != -1000.0 && h > 0.0 && w > 0.0 && l > 0.0) atomicOr(&flags[7 + c], 1);   // :185
}

// toPolygon (:289-311): l along x, w along z, rotated by ry; made counter-clockwise for the clip.  Returns the footprint's area.
__device__ __forceinline__ double footprint(double l, double w, double ry, double t1, double t3, double (&px)[4], double (&pz)[4]) {
    const double c = cos(ry), s = sin(ry);
    const double hx[4] = {l / 2, l / 2, -l / 2, -l / 2}, hz[4] = {w / 2, -w / 2, -w / 2, w / 2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = (c * hx[k] + s * hz[k]) + t1;
        pz[k] = (-s * hx[k] + c * hz[k]) + t3;
    }
    double a2 = twice_area(px, pz);
    if (a2 < 0.0) {
        double t = px[1]; px[1] = px[3]; px[3] = t;
        t = pz[1]; pz[1] = pz[3]; pz[3] = t;
        a2 = twice_area(px, pz);
    }
    return 0.5 * a2;
}

__device__ __forceinline__ double min4(const double (&v)[4]) { return fmin(fmin(v[0], v[1]), fmin(v[2], v[3])); }
__device__ __forceinline__ double max4(const double (&v)[4]) { return fmax(fmax(v[0], v[1]), fmax(v[2], v[3])); }

// the three overlap functions of one (detection, ground truth) pair; criterion -1: over the union, 0: over the detection
__device__ __forceinline__ void pair_overlaps(const double* __restrict__ d, const double* __restrict__ g, int criterion, double& o_img,
                                              double& o_gnd, double& o_3d) {
    {   // imageBoxOverlap (:247-281)
        const double ax1 = d[GNMS_KITTI_DET_X1], ay1 = d[GNMS_KITTI_DET_X1 + 1], ax2 = d[GNMS_KITTI_DET_X1 + 2], ay2 = d[GNMS_KITTI_DET_X1 + 3];
        const double bx1 = g[GNMS_KITTI_GT_X1], by1 = g[GNMS_KITTI_GT_X1 + 1], bx2 = g[GNMS_KITTI_GT_X1 + 2], by2 = g[GNMS_KITTI_GT_X1 + 3];
        const double x1 = ax1 > bx1 ? ax1 : bx1, y1 = ay1 > by1 ? ay1 : by1, x2 = ax2 < bx2 ? ax2 : bx2, y2 = ay2 < by2 ? ay2 : by2;
        const double w = x2 - x1, h = y2 - y1;
        if (w <= 0.0 || h <= 0.0) {
            o_img = 0.0;
        } else {
            const double inter = w * h, a_area = (ax2 - ax1) * (ay2 - ay1), b_area = (bx2 - bx1) * (by2 - by1);
            o_img = criterion == -1 ? inter / (a_area + b_area - inter) : inter / a_area;
        }
    }
    // groundBoxOverlap / box3DOverlap (:314-364)
    const double dh = d[GNMS_KITTI_DET_H], dw = d[GNMS_KITTI_DET_H + 1], dl = d[GNMS_KITTI_DET_H + 2];
    const double gh = g[GNMS_KITTI_GT_H], gw = g[GNMS_KITTI_GT_H + 1], gl = g[GNMS_KITTI_GT_H + 2];
    const double dt2 = d[GNMS_KITTI_DET_T + 1], gt2 = g[GNMS_KITTI_GT_T + 1];
    double dx[4], dz[4], gx[4], gz[4];
    const double d_area = footprint(dl, dw, d[GNMS_KITTI_DET_RY], d[GNMS_KITTI_DET_T], d[GNMS_KITTI_DET_T + 2], dx, dz);
    const double g_area = footprint(gl, gw, g[GNMS_KITTI_GT_RY], g[GNMS_KITTI_GT_T], g[GNMS_KITTI_GT_T + 2], gx, gz);
    double inter = 0.0;
    const bool xz = fmax(min4(dx), min4(gx)) < fmin(max4(dx), max4(gx)) && fmax(min4(dz), min4(gz)) < fmin(max4(dz), max4(gz));
    if (xz && d_area > 0.0 && g_area > 0.0) {
        const double ox = dx[0], oz = dz[0];
        double ax[4], az[4], bx[4], bz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ax[q] = dx[q] - ox; az[q] = dz[q] - oz; bx[q] = gx[q] - ox; bz[q] = gz[q] - oz; }
        inter = intersection_area(ax, az, bx, bz);
    }
    o_gnd = criterion == -1 ? inter / ((d_area + g_area) - inter) : inter / d_area;
    const double ymax = dt2 < gt2 ? dt2 : gt2;                                                   // :346 (t2 is the bottom face)
    const double ylo_d = dt2 - dh, ylo_g = gt2 - gh;
    const double ymin = ylo_d > ylo_g ? ylo_d : ylo_g;
    const double dy = ymax - ymin;
    const double inter_vol = inter * (0.0 > dy ? 0.0 : dy);
    const double det_vol = dh * dl * dw, gt_vol = gh * gl * gw;
    o_3d = criterion == -1 ? inter_vol / (det_vol + gt_vol - inter_vol) : inter_vol / det_vol;
}

__global__ __launch_bounds__(256) void overlaps_kernel(const double* __restrict__ det, const double* __restrict__ gt,
                                                       const int32_t* __restrict__ det_off, const int32_t* __restrict__ gt_off,
                                                       const int64_t* __restrict__ pair_off, int64_t n_pairs, double* __restrict__ ov) {
    const int img = blockIdx.x;
    const int d0 = det_off[img], nd = det_off[img + 1] - d0, g0 = gt_off[img], ng = gt_off[img + 1] - g0;
    const int64_t p0 = pair_off[img];
    const int count = nd * ng;
    for (int p = threadIdx.x; p < count; p += blockDim.x) {
        const int g = p / nd, j = p - g * nd;
        if (p0 + p >= n_pairs) break;
        const double* grow = gt + (size_t)(g0 + g) * kGtCols;
        const int criterion = grow[GNMS_KITTI_GT_TYPE] == (double)T_DC ? 0 : -1;
        double a, b, c;
        pair_overlaps(det + (size_t)(d0 + j) * kDetCols, grow, criterion, a, b, c);
        ov[p0 + p] = a;
        ov[n_pairs + p0 + p] = b;
        ov[2 * n_pairs + p0 + p] = c;
    }
}

// One image of one curve, as seen by one lane.
struct Image {
    const double* det; const double* gt; const double* ov;      // rows of the image; ov[g * nd + j] of the curve's metric
    int nd, ng;
};

// cleanData (:401-474), per row
__device__ __forceinline__ int ignored_gt_of(const double* __restrict__ g, int cls, int diff, double max_depth) {
    const int type = (int)g[GNMS_KITTI_GT_TYPE];
    const double height = g[GNMS_KITTI_GT_X1 + 3] - g[GNMS_KITTI_GT_X1 + 1];                     // :407
    int valid_class;
    if (type == cls) valid_class = 1;                                                            // :414
    else if (cls == T_PED && type == T_SIT) valid_class = 0;                                     // :418
    else if (cls == T_CAR && type == T_VAN) valid_class = 0;                                     // :420
    else valid_class = -1;
    const bool ignore = g[GNMS_KITTI_GT_OCC] > (double)max_occlusion(diff) || g[GNMS_KITTI_GT_TRUNC] > max_truncation(diff) ||
                        height <= (double)min_height(diff) || g[GNMS_KITTI_GT_T + 2] > max_depth;   // :430 (|| gt.t3 > D in the variants)
    if (valid_class == 1 && !ignore) return 0;
    if (valid_class == 0 || (ignore && valid_class == 1)) return 1;
    return -1;
}
__device__ __forceinline__ int ignored_det_of(const double* __restrict__ d, int cls, int diff) {
    const int height = (int)fabs(d[GNMS_KITTI_DET_X1 + 1] - d[GNMS_KITTI_DET_X1 + 3]);           // :464 int32_t height = fabs(...)
    if (height < min_height(diff)) return 1;
    return (int)d[GNMS_KITTI_DET_CLASS] == cls && d[GNMS_KITTI_DET_CLASS] >= 0.0 ? 0 : -1;
}

struct Stat { int tp, fp, fn, n_gt; double similarity; };

// computeStatistics (:476-634).  asg: the lane's assigned_detection words, asg[w * 64].  FP = compute_fp.  Without FP, tp_slot (if
// not NULL) receives per ground-truth row the score of its true positive or -inf (stat.v, :564).
template <bool FP>
__device__ __forceinline__ Stat compute_statistics(const Image& im, int cls, int diff, double min_overlap, double max_depth, bool compute_aos,
                                                   double thresh, unsigned long long* asg, double* tp_slot) {
    const double NO_DETECTION = -10000000;
    Stat st = {0, 0, 0, 0, 0.0};
    const int nw = (im.nd + 63) >> 6;
    for (int w = 0; w < nw; ++w) asg[w * 64] = 0ull;
    for (int i = 0; i < im.ng; ++i) {
        const double* g = im.gt + (size_t)i * kGtCols;
        const int ign_gt = ignored_gt_of(g, cls, diff, max_depth);
        if (ign_gt == 0) st.n_gt++;                                                              // :437
        if (!FP && tp_slot) tp_slot[i] = -__builtin_inf();
        if (ign_gt == -1) continue;                                                              // :500
        int det_idx = -1;
        double valid_detection = NO_DETECTION, max_overlap = 0.0;
        bool assigned_ignored_det = false;
        const double* orow = im.ov + (size_t)i * im.nd;
        unsigned long long word = 0ull;
        for (int j = 0; j < im.nd; ++j) {
            if ((j & 63) == 0) word = asg[(j >> 6) * 64];
            const double* d = im.det + (size_t)j * kDetCols;
            const int ign_det = ignored_det_of(d, cls, diff);
            if (ign_det == -1) continue;                                                         // :515
            if ((word >> (j & 63)) & 1ull) continue;                                             // :517
            const double score = d[GNMS_KITTI_DET_SCORE];
            if (FP && score < thresh) continue;                                                  // :493, :519
            const double overlap = orow[j];
            if (!FP) {
                if (overlap > min_overlap && score > valid_detection) {                          // :526
                    det_idx = j;
                    valid_detection = score;
                }
            } else if (overlap > min_overlap && (overlap > max_overlap || assigned_ignored_det) && ign_det == 0) {   // :533
                max_overlap = overlap;
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = false;
            } else if (overlap > min_overlap && valid_detection == NO_DETECTION && ign_det == 1) {   // :539
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = true;
            }
        }
        if (valid_detection == NO_DETECTION) {
            if (ign_gt == 0) st.fn++;                                                            // :551
            continue;
        }
        const double* dbest = im.det + (size_t)det_idx * kDetCols;
        if (!(ign_gt == 1 || ignored_det_of(dbest, cls, diff) == 1)) {                           // :556 else :560
            st.tp++;
            if (!FP && tp_slot) tp_slot[i] = dbest[GNMS_KITTI_DET_SCORE];
            if (FP && compute_aos) st.similarity += (1.0 + cos(g[GNMS_KITTI_GT_ALPHA] - dbest[GNMS_KITTI_DET_ALPHA])) / 2.0;   // :568, :618
        }
        asg[(det_idx >> 6) * 64] |= 1ull << (det_idx & 63);                                      // :557, :571
    }
    if (FP) {
        unsigned long long word = 0ull;
        for (int j = 0; j < im.nd; ++j) {                                                        // :579-584
            if ((j & 63) == 0) word = asg[(j >> 6) * 64];
            const double* d = im.det + (size_t)j * kDetCols;
            if (!(((word >> (j & 63)) & 1ull) || ignored_det_of(d, cls, diff) != 0 || d[GNMS_KITTI_DET_SCORE] < thresh)) st.fp++;
        }
        int nstuff = 0;
        for (int i = 0; i < im.ng; ++i) {                                                        // :588 (dc: the DontCare rows, in order)
            if (im.gt[(size_t)i * kGtCols + GNMS_KITTI_GT_TYPE] != (double)T_DC) continue;
            const double* orow = im.ov + (size_t)i * im.nd;
            for (int j = 0; j < im.nd; ++j) {
                const unsigned long long bit = 1ull << (j & 63);
                if (asg[(j >> 6) * 64] & bit) continue;
                const double* d = im.det + (size_t)j * kDetCols;
                if (ignored_det_of(d, cls, diff) != 0) continue;
                if (d[GNMS_KITTI_DET_SCORE] < thresh) continue;
                if (orow[j] > min_overlap) {                                                     // :600-604
                    asg[(j >> 6) * 64] |= bit;
                    nstuff++;
                }
            }
        }
        st.fp -= nstuff;                                                                         // :609
        // :612-631: the image's similarity is the sum above (the fp zeros add nothing; with tp = fp = 0 the sum is empty)
    }
    return st;
}

__device__ __forceinline__ bool curve_on(const int* __restrict__ flags, int curve) {
    const int cls = curve / 9, metric = (curve / 3) % 3;
    return flags[1 + 3 * metric + cls] != 0;
}

__device__ __forceinline__ Image image_of(const double* det, const double* gt, const int32_t* det_off, const int32_t* gt_off,
                                          const int64_t* pair_off, const double* ov, int64_t n_pairs, int img, int metric) {
    Image im;
    const int d0 = det_off[img], g0 = gt_off[img];
    im.nd = min(det_off[img + 1] - d0, kMaxDet);
    im.ng = gt_off[img + 1] - g0;
    im.det = det + (size_t)d0 * kDetCols;
    im.gt = gt + (size_t)g0 * kGtCols;
    im.ov = ov + (size_t)metric * n_pairs + pair_off[img];
    return im;
}

// lane = (variant, curve) task of image blockIdx.x
__global__ __launch_bounds__(64) void recall_kernel(const double* __restrict__ det, const double* __restrict__ gt,
                                                    const int32_t* __restrict__ det_off, const int32_t* __restrict__ gt_off,
                                                    const int64_t* __restrict__ pair_off, const double* __restrict__ ov, int64_t n_pairs,
                                                    int n_gt_rows, const int* __restrict__ flags, const double* __restrict__ vmin,
                                                    const double* __restrict__ vdepth, int V, double* __restrict__ tp_scores,
                                                    int* __restrict__ n_tp, int* __restrict__ n_gt) {
    __shared__ unsigned long long asg[kWords][64];
    const int img = blockIdx.x, task = blockIdx.y * 64 + threadIdx.x;
    if (task >= V * kCurves) return;
    const int v = task / kCurves, curve = task % kCurves;
    if (!curve_on(flags, curve)) return;
    const int cls = curve / 9, metric = (curve / 3) % 3, diff = curve % 3;
    const Image im = image_of(det, gt, det_off, gt_off, pair_off, ov, n_pairs, img, metric);
    double* slot = tp_scores + (size_t)task * n_gt_rows + gt_off[img];
    const Stat st = compute_statistics<false>(im, cls, diff, vmin[v * 9 + metric * 3 + cls], vdepth[v], false, 0.0, &asg[0][threadIdx.x], slot);
    if (st.tp) atomicAdd(&n_tp[task], st.tp);
    if (st.n_gt) atomicAdd(&n_gt[task], st.n_gt);
}

// getThresholds (:366-399) on the sorted row; lane = curve task.  No more than 41 thresholds can come out while the number of true
// positives does not exceed n_gt (which the recall pass guarantees: a true positive needs a ground truth of its own): the 41st
// push needs (2 i + 3) / n_gt >= 2, i.e. i >= n_gt - 1, which only the last score can satisfy.  The store is bounded all the same.
__global__ __launch_bounds__(64) void thresholds_kernel(const double* __restrict__ sorted, int n_gt_rows, const int* __restrict__ n_tp,
                                                        const int* __restrict__ n_gt, int tasks, double* __restrict__ thr,
                                                        int* __restrict__ n_thr) {
    const int task = blockIdx.x * 64 + threadIdx.x;
    if (task >= tasks) return;
    const double* v = sorted + (size_t)task * n_gt_rows;
    const int n = min(n_tp[task], n_gt_rows);
    const double n_groundtruth = (double)n_gt[task];
    double current_recall = 0.0;
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const double l_recall = (double)(i + 1) / n_groundtruth;
        const double r_recall = i < n - 1 ? (double)(i + 2) / n_groundtruth : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
        if (count < kPts) thr[(size_t)task * kPts + count] = v[i];
        ++count;
        current_recall += 1.0 / (41.0 - 1.0);
    }
    n_thr[task] = min(count, kPts);
}

// one wave per (image, curve task); lane t = threshold t
__global__ __launch_bounds__(64) void precision_kernel(const double* __restrict__ det, const double* __restrict__ gt,
                                                       const int32_t* __restrict__ det_off, const int32_t* __restrict__ gt_off,
                                                       const int64_t* __restrict__ pair_off, const double* __restrict__ ov, int64_t n_pairs,
                                                       int I, const int* __restrict__ flags, const double* __restrict__ vmin,
                                                       const double* __restrict__ vdepth, const double* __restrict__ thr,
                                                       const int* __restrict__ n_thr, int* __restrict__ counts, double* __restrict__ sim) {
    __shared__ unsigned long long asg[kWords][64];
    const int img = blockIdx.x, task = blockIdx.y, t = threadIdx.x;
    const int v = task / kCurves, curve = task % kCurves;
    if (!curve_on(flags, curve) || t >= n_thr[task]) return;
    const int cls = curve / 9, metric = (curve / 3) % 3, diff = curve % 3;
    const bool compute_aos = metric == 0 && flags[0] == 0;                                       // :809, :882
    const Image im = image_of(det, gt, det_off, gt_off, pair_off, ov, n_pairs, img, metric);
    const Stat st = compute_statistics<true>(im, cls, diff, vmin[v * 9 + metric * 3 + cls], vdepth[v], compute_aos,
                                             thr[(size_t)task * kPts + t], &asg[0][t], nullptr);
    int* c = counts + ((size_t)task * kPts + t) * 3;
    if (st.tp) atomicAdd(c, st.tp);                                                              // :692-694
    if (st.fp) atomicAdd(c + 1, st.fp);
    if (st.fn) atomicAdd(c + 2, st.fn);
    if (compute_aos) sim[(((size_t)v * 9 + cls * 3 + diff) * I + img) * kPts + t] = st.similarity;
}

// one wave per curve task: :700-719
__global__ __launch_bounds__(64) void finish_kernel(int I, const int* __restrict__ flags, const int* __restrict__ n_thr,
                                                    const int* __restrict__ counts, const double* __restrict__ sim,
                                                    double* __restrict__ precision, double* __restrict__ aos) {
    __shared__ double p[kPts], a[kPts];
    const int task = blockIdx.x, t = threadIdx.x;
    const int v = task / kCurves, curve = task % kCurves;
    const int cls = curve / 9, metric = (curve / 3) % 3, diff = curve % 3;
    const bool on = curve_on(flags, curve), compute_aos = on && metric == 0 && flags[0] == 0;
    const int n = on ? n_thr[task] : 0;
    if (t < kPts) {
        double pr = 0.0, ao = 0.0;
        if (t < n) {
            const int* c = counts + ((size_t)task * kPts + t) * 3;
            const double denom = (double)(c[0] + c[1]);
            pr = (double)c[0] / denom;                                                           // :709 (0 / 0 stays the IEEE NaN)
            if (compute_aos) {
                const double* s = sim + ((size_t)v * 9 + cls * 3 + diff) * I * kPts + t;
                double sum = 0.0;
                for (int img = 0; img < I; ++img) sum += s[(size_t)img * kPts];                  // :696, in image order
                ao = sum / denom;                                                                // :711
            }
        }
        p[t] = pr;
        a[t] = ao;
    }
    __syncthreads();
    if (t < kPts) {
        // :715-719, *max_element(begin + i, end): the first element no later one exceeds.  Entries i < t were replaced before
        // entry t is, but element t's range starts at t: it reads raw values only.
        double bp = p[t], ba = a[t];
        for (int k = t + 1; k < kPts; ++k) {
            if (bp < p[k]) bp = p[k];
            if (ba < a[k]) ba = a[k];
        }
        const bool live = t < n;
        precision[(size_t)task * kPts + t] = live ? bp : 0.0;
        if (metric == 0) aos[((size_t)v * 9 + cls * 3 + diff) * kPts + t] = (live && compute_aos) ? ba : 0.0;
    }
}

}  // namespace

extern "C" int gnms_kitti_eval_plan(const int32_t* det_offsets_host, const int32_t* gt_offsets_host, int I, int V, int64_t* n_pairs) {
    GNMS_CHECK_ARG(I >= 0, "gnms_kitti_eval_plan: negative image count (%d)", I);
    GNMS_CHECK_ARG(V >= 1, "gnms_kitti_eval_plan: needs at least one variant (V=%d)", V);
    GNMS_CHECK_ARG(det_offsets_host && gt_offsets_host && n_pairs, "gnms_kitti_eval_plan: null pointer");
    GNMS_CHECK_ARG(det_offsets_host[0] == 0 && gt_offsets_host[0] == 0, "gnms_kitti_eval_plan: offsets must start at 0");
    GNMS_CHECK_ARG((int64_t)V * GNMS_KITTI_EVAL_CURVES <= 65535, "gnms_kitti_eval_plan: too many variants (%d)", V);
    int64_t pairs = 0;
    for (int i = 0; i < I; ++i) {
        const int64_t nd = (int64_t)det_offsets_host[i + 1] - det_offsets_host[i], ng = (int64_t)gt_offsets_host[i + 1] - gt_offsets_host[i];
        GNMS_CHECK_ARG(nd >= 0 && ng >= 0, "gnms_kitti_eval_plan: offsets not ascending at image %d", i);
        GNMS_CHECK_ARG(nd <= GNMS_KITTI_EVAL_MAX_DET, "gnms_kitti_eval_plan: image %d has %lld detections, the limit is %d", i, (long long)nd,
                       GNMS_KITTI_EVAL_MAX_DET);
        GNMS_CHECK_ARG(ng <= GNMS_KITTI_EVAL_MAX_GT, "gnms_kitti_eval_plan: image %d has %lld ground-truth rows, the limit is %d", i,
                       (long long)ng, GNMS_KITTI_EVAL_MAX_GT);
        pairs += nd * ng;
    }
    *n_pairs = pairs;
    return GNMS_OK;
}

extern "C" int gnms_kitti_eval_recall(const double* det, const double* gt, const int32_t* det_offsets, const int32_t* gt_offsets,
                                      const int64_t* pair_offsets, int I, int n_det, int n_gt_rows, int64_t n_pairs,
                                      const double* min_overlap, const double* max_depth, int V, double* overlaps, int32_t* flags,
                                      double* tp_scores, int32_t* n_tp, int32_t* n_gt, void* stream) {
    GNMS_CHECK_ARG(I >= 0 && n_det >= 0 && n_gt_rows >= 0 && n_pairs >= 0, "gnms_kitti_eval_recall: negative count (I=%d n_det=%d n_gt=%d)", I, n_det,
                   n_gt_rows);
    GNMS_CHECK_ARG(V >= 1 && (int64_t)V * kCurves <= 65535, "gnms_kitti_eval_recall: V (%d) out of range", V);
    GNMS_CHECK_ARG(det_offsets && gt_offsets && pair_offsets && min_overlap && max_depth && flags && n_tp && n_gt,
                   "gnms_kitti_eval_recall: null pointer");
    GNMS_CHECK_ARG((det || n_det == 0) && (gt || n_gt_rows == 0) && (overlaps || n_pairs == 0) && (tp_scores || n_gt_rows == 0),
                   "gnms_kitti_eval_recall: null array");
    hipStream_t st = (hipStream_t)stream;
    const int tasks = V * kCurves;
    GNMS_CHECK_HIP(hipMemsetAsync(flags, 0, kFlags * sizeof(int32_t), st));
    GNMS_CHECK_HIP(hipMemsetAsync(n_tp, 0, tasks * sizeof(int32_t), st));
    GNMS_CHECK_HIP(hipMemsetAsync(n_gt, 0, tasks * sizeof(int32_t), st));
    if (n_det > 0) {
        flags_kernel<<<gnms_div_up(n_det, 256), 256, 0, st>>>(det, n_det, flags);
        GNMS_CHECK_LAUNCH();
    }
    if (I == 0) return GNMS_OK;
    if (n_pairs > 0) {
        overlaps_kernel<<<I, 256, 0, st>>>(det, gt, det_offsets, gt_offsets, pair_offsets, n_pairs, overlaps);
        GNMS_CHECK_LAUNCH();
    }
    recall_kernel<<<dim3(I, gnms_div_up(tasks, 64)), 64, 0, st>>>(det, gt, det_offsets, gt_offsets, pair_offsets, overlaps, n_pairs, n_gt_rows,
                                                                  flags, min_overlap, max_depth, V, tp_scores, n_tp, n_gt);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_kitti_eval_precision(const double* det, const double* gt, const int32_t* det_offsets, const int32_t* gt_offsets,
                                         const int64_t* pair_offsets, int I, int n_gt_rows, int64_t n_pairs, const double* min_overlap,
                                         const double* max_depth, int V, const double* overlaps, const int32_t* flags,
                                         const double* sorted_scores, const int32_t* n_tp, const int32_t* n_gt, double* thresholds,
                                         int32_t* n_thresholds, int32_t* counts, double* similarity, double* precision, double* aos,
                                         void* stream) {
    GNMS_CHECK_ARG(I >= 0 && n_gt_rows >= 0 && n_pairs >= 0, "gnms_kitti_eval_precision: negative count (I=%d n_gt=%d)", I, n_gt_rows);
    GNMS_CHECK_ARG(V >= 1 && (int64_t)V * kCurves <= 65535, "gnms_kitti_eval_precision: V (%d) out of range", V);
    GNMS_CHECK_ARG(det_offsets && gt_offsets && pair_offsets && min_overlap && max_depth && flags && n_tp && n_gt && thresholds && n_thresholds &&
                       counts && precision && aos,
                   "gnms_kitti_eval_precision: null pointer");
    GNMS_CHECK_ARG((sorted_scores || n_gt_rows == 0) && (similarity || I == 0) && (overlaps || n_pairs == 0) && (gt || n_gt_rows == 0),
                   "gnms_kitti_eval_precision: null array");
    hipStream_t st = (hipStream_t)stream;
    const int tasks = V * kCurves;
    GNMS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)tasks * kPts * 3 * sizeof(int32_t), st));
    GNMS_CHECK_HIP(hipMemsetAsync(thresholds, 0, (size_t)tasks * kPts * sizeof(double), st));
    thresholds_kernel<<<gnms_div_up(tasks, 64), 64, 0, st>>>(sorted_scores, n_gt_rows, n_tp, n_gt, tasks, thresholds, n_thresholds);
    GNMS_CHECK_LAUNCH();
    if (I > 0) {
        precision_kernel<<<dim3(I, tasks), 64, 0, st>>>(det, gt, det_offsets, gt_offsets, pair_offsets, overlaps, n_pairs, I, flags, min_overlap,
                                                        max_depth, thresholds, n_thresholds, counts, similarity);
        GNMS_CHECK_LAUNCH();
    }
    finish_kernel<<<tasks, 64, 0, st>>>(I, flags, n_thresholds, counts, similarity, precision, aos);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
