// after_nms.hip -- the after-NMS block of the reference's RPN loss (lib/loss/rpn_3d.py:721-825, :1091-1148) around the pieces the
// library already has (gnms_select_topk, the layer, gnms_best_targets, the AP loss).  DESIGN.md 3.16.
//
//   gnms_after_nms_decode   one launch over (ceil(max(K, M) / 256), B): lane k < K gathers the rows of selected anchor sel_index[b][k]
//                           and decodes its 2D box (bbox_decode.h, the arithmetic of gnms_bbox_transform_inv) and its camera-space
//                           cuboid (:318-363, :532-574, fp32 in the reference's operation order); lane m < M repacks ground truth m
//                           of the image into the (x y z w h l ry) / (x1 y1 x2 y2) rows gnms_best_targets takes.  Rows behind an
//                           image's count are zero.  Only the selected anchors are touched.
//   gnms_after_nms_finish   one workgroup.  phase 0 (in front of the AP loss): the zero tail of every image, fg_counts - sel_counts,
//                           the targets from gnms_best_targets' index per ground truth, and the [B * K] targets with -1 on the padding that the all-images-at-once ranking reads as one row.
//                           phase 1 (behind it): img_cnt, the scalar loss, and d loss / d (rescored probability) with lambda and
//                           1 / img_cnt folded in; in mode "classify" the weighted binary cross entropy itself.
//   gnms_after_nms_scatter  over (ceil(R / 256), B): every workgroup zeroes the gradient rows of its 256 anchors, then writes the
//                           selected anchors that fall among them (indices within an image are unique).  Plain vector stores, no
//                           global atomics, no workgroup waits for another.
#include <math.h>
#include "gnms_common.h"
#include "bbox_decode.h"

namespace {

constexpr int AN_THREADS = 256;
constexpr int AN_WAVES = AN_THREADS / GNMS_WAVE;
constexpr int AN_SNAP_TRIPS = 1024;              // trip bound of the snap_to_pi loops (csrc/kitti_rows.hip)

struct DecodeArgs {
    const int64_t* sel_index;    // [B][K]
    const int32_t* sel_counts;   // [B]
    const float* b2;             // [B][R][4]
    const float* b3;             // [B][R][ld_b3]
    const float* gt;             // [B][R] rows of ld_gt (raw_gt: 19 = axis label, 20 = head label)
    const float* rois;           // [B][R] rows of ld_rois
    const float* r3;             // [B][R] rows of ld_r3
    const float* cen;            // [B][R][2]
    const double* p2;            // [B][p2_rows][4]
    const double* scale;         // [B]
    const double* gts_val;       // [B][M][4]
    const double* gts_3d;        // [B][M][ld_g3]
    const int32_t* val_counts;   // [B]
    int ld_b3, ld_rois, ld_r3, p2_rows, ld_g3;
    long long ld_gt;
    int B, K, R, M;
    float means[13], stds[13];
    float* boxes;                // [B][K][4]
    float* cuboids;              // [B][K][7]
    float* gt_params;            // [B][M][7]
    float* gt_boxes;             // [B][M][4]
};

// math_3d.py:497-510 / util.py:637-638 in fp32, as the reference's tensors are; bounded, and a non-finite angle stays as it is
__device__ __forceinline__ float snap_to_pi_f(float a) {
    const float pi = (float)3.141592653589793, two_pi = (float)(2.0 * 3.141592653589793);
    if (!isfinite(a)) return a;
    for (int i = 0; i < AN_SNAP_TRIPS && a > pi; ++i) a -= two_pi;
    for (int i = 0; i < AN_SNAP_TRIPS && a <= -pi; ++i) a += two_pi;
    return a;
}

__global__ __launch_bounds__(AN_THREADS) void after_nms_decode_kernel(DecodeArgs a) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * AN_THREADS + threadIdx.x;
    if (i < a.K) {
        const int cnt = min(max(a.sel_counts[b], 0), a.K);
        const long long out = (long long)b * a.K + i;
        float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float c[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const long long r = i < cnt ? (long long)a.sel_index[out] : -1;
        if (r >= 0 && r < a.R) {
            const long long row = (long long)b * a.R + r;
            const float* roi = a.rois + row * a.ld_rois;
            const float* b3 = a.b3 + row * a.ld_b3;
            const float* r3 = a.r3 + row * a.ld_r3;
            const float* gt = a.gt + row * a.ld_gt;
            const float4 anchor = make_float4(roi[0], roi[1], roi[2], roi[3]);
            const float4 d = reinterpret_cast<const float4*>(a.b2)[row];
            box = gnms_bbox_decode(anchor, d, make_float4(a.means[0], a.means[1], a.means[2], a.means[3]),
                                   make_float4(a.stds[0], a.stds[1], a.stds[2], a.stds[3]), 1, 1);        // :316
            const float widths = anchor.z - anchor.x + 1.0f;                                               // :338
            const float heights = anchor.w - anchor.y + 1.0f;                                              // :339
            const float x_dn = (b3[0] * a.stds[4] + a.means[4]) * widths + a.cen[row * 2 + 0];             // :318, :351
            const float y_dn = (b3[1] * a.stds[5] + a.means[5]) * heights + a.cen[row * 2 + 1];            // :319, :352
            const float z_dn = r3[4] + (b3[2] * a.stds[6] + a.means[6]);                                   // :320, :354
            c[3] = expf(b3[3] * a.stds[7] + a.means[7]) * r3[5];                                           // :355
            c[4] = expf(b3[4] * a.stds[8] + a.means[8]) * r3[6];                                           // :356
            c[5] = expf(b3[5] * a.stds[9] + a.means[9]) * r3[7];                                           // :357
            const float rsin = r3[9] + (b3[6] * a.stds[11] + a.means[11]);                                 // :327, :362
            const float rcos = r3[10] + (b3[7] * a.stds[12] + a.means[12]);                                // :328, :363
            const double* P = a.p2 + (long long)b * a.p2_rows * 4;
            const float pa = (float)P[0], pb = (float)P[2], pc = (float)P[3], pd = (float)P[5], pe = (float)P[6], pf = (float)P[7], ph = (float)P[11];
            const float sc = (float)a.scale[b];
            const float x_2d = x_dn / sc, y_2d = y_dn / sc;                                                // :532-533
            const float z_raw = z_dn - ph;                                                                 // :553
            const float x_raw = ((z_raw + ph) * x_2d - pb * z_raw - pc) / pa;                              // :554
            const float y_raw = ((z_raw + ph) * y_2d - pe * z_raw - pf) / pd;                              // :555
            float rot = gt[19] == 1.0f ? rsin : rcos;                                                      // :569-570
            if (gt[20] == 1.0f) rot = rot + (float)3.141592653589793;                                      // :571
            const float alpha = snap_to_pi_f(rot);                                                         // :573
            const float ry = snap_to_pi_f(alpha + atan2f(-z_raw, x_raw) + (float)(0.5 * 3.141592653589793));   // :574, util.py:635-638
            c[0] = x_raw; c[1] = y_raw; c[2] = z_raw; c[6] = ry;
        }
        reinterpret_cast<float4*>(a.boxes)[out] = box;
#pragma unroll
        for (int k = 0; k < 7; ++k) a.cuboids[out * 7 + k] = c[k];
    }
    if (i < a.M) {
        const int cnt = min(max(a.val_counts[b], 0), a.M);
        const long long m = (long long)b * a.M + i;
        float4 gb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float g[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (i < cnt) {
            const double* v = a.gts_val + m * 4;
            const double* q = a.gts_3d + m * a.ld_g3;
            gb = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);                          // :801
            g[0] = (float)q[7]; g[1] = (float)q[8]; g[2] = (float)q[9]; g[3] = (float)q[3]; g[4] = (float)q[4]; g[5] = (float)q[5];
            g[6] = (float)q[10];                                                                           // :805-811
        }
        reinterpret_cast<float4*>(a.gt_boxes)[m] = gb;
#pragma unroll
        for (int k = 0; k < 7; ++k) a.gt_params[m * 7 + k] = g[k];
    }
}

struct FinishArgs {
    int phase, mode;             // mode: 0 rank per image, 1 rank all images at once, 2 classify
    int B, K;
    const int32_t* fg_counts;    // [B]
    const int32_t* sel_counts;   // [B]
    const float* prob;           // [B][K] rescored probabilities
    float* targets;              // [B][K]: written by phase 0 from best_index, read by phase 1
    const int64_t* best_index;   // [B][M] (gnms_best_targets): the selected box that is ground truth m's best, or -1
    int M;
    const float* ap_loss;        // [B] (mode 1: [1])
    const float* ap_grad;        // [B][K]
    float lambda;
    int32_t* tail_counts;        // [B + 1]: per image, then the batch's total
    float* targets_padded;       // [B][K]
    float* loss;                 // [2 + B]: the loss, the statistic, the per-image losses
    int32_t* img_cnt;            // [1]
    float* dprob;                // [B][K]
};

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int s = 1; s < GNMS_WAVE; s <<= 1) v += __shfl_xor(v, s);
    __syncthreads();
    if ((threadIdx.x & (GNMS_WAVE - 1)) == 0) red[threadIdx.x / GNMS_WAVE] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < AN_WAVES; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(AN_THREADS) void after_nms_finish_kernel(FinishArgs a) {
    __shared__ double red[AN_WAVES];
    const int t = threadIdx.x;
    const int total = a.B * a.K;
    if (a.phase == 0) {
        // targets_after_nms (:825): 1 on a box that some ground truth chose, with plain stores (several ground truths may choose one box)
        for (int i = t; i < total; i += AN_THREADS) {
            const int b = i / a.K, k = i - b * a.K;
            const bool live = k < min(max(a.sel_counts[b], 0), a.K);
            float v = 0.0f;
            if (live)
                for (int m = 0; m < a.M; ++m) v = a.best_index[(long long)b * a.M + m] == (long long)k ? 1.0f : v;
            a.targets[i] = v;
            a.targets_padded[i] = live ? v : -1.0f;
        }
        if (t == 0) {
            long long sum = 0;
            for (int b = 0; b < a.B; ++b) {
                const int e = max(a.fg_counts[b] - min(max(a.sel_counts[b], 0), a.K), 0);
                a.tail_counts[b] = e;
                sum += e;
            }
            a.tail_counts[a.B] = (int)min(sum, (long long)2147483647);
        }
        return;
    }
    int cnt = 0;                                           // images with sampled foreground (:1124-1125)
    long long fg_total = 0;
    for (int b = 0; b < a.B; ++b) { cnt += a.fg_counts[b] > 0 ? 1 : 0; fg_total += max(a.fg_counts[b], 0); }
    if (a.mode == 2) {
        // :1103-1115; the zero tail (score 0, target 0) counts in n_neg and in the mean, and its terms are 0
        double npos = 0.0, nneg = 0.0;
        for (int i = t; i < total; i += AN_THREADS) {
            const int b = i / a.K, k = i - b * a.K;
            if (k < min(max(a.sel_counts[b], 0), a.K)) { npos += a.targets[i] == 1.0f ? 1.0 : 0.0; nneg += a.targets[i] == 0.0f ? 1.0 : 0.0; }
        }
        npos = block_sum(npos, red);
        nneg = block_sum(nneg, red);
        long long tail = 0;
        for (int b = 0; b < a.B; ++b) tail += max(a.fg_counts[b] - min(max(a.sel_counts[b], 0), a.K), 0);
        nneg += (double)tail;
        const double wneg = (npos > 0.0 && nneg > 0.0) ? (double)(float)pow(npos / nneg, 0.25) : 1.0;     // :1109-1111
        double sum = 0.0, nfin = 0.0;
        for (int i = t; i < total; i += AN_THREADS) {
            const int b = i / a.K, k = i - b * a.K;
            if (k < min(max(a.sel_counts[b], 0), a.K)) {
                const double p = (double)a.prob[i], y = (double)a.targets[i];
                double lp = log(p), lq = log(1.0 - p);
                lp = lp < -100.0 ? -100.0 : lp;
                lq = lq < -100.0 ? -100.0 : lq;
                const double v = (a.targets[i] == 0.0f ? wneg : 1.0) * ((y - 1.0) * lq - y * lp);           // :1112-1113
                if (isfinite(v)) { sum += v; nfin += 1.0; }
            }
        }
        sum = block_sum(sum, red);
        nfin = block_sum(nfin, red) + (double)tail;
        const double mean = fg_total > 0 ? sum / nfin : 0.0;                                               // :1100-1101, :1115
        for (int i = t; i < total; i += AN_THREADS) {
            const int b = i / a.K, k = i - b * a.K;
            float g = 0.0f;
            if (fg_total > 0 && k < min(max(a.sel_counts[b], 0), a.K)) {
                const double p = (double)a.prob[i], y = (double)a.targets[i];
                double lp = log(p), lq = log(1.0 - p);
                lp = lp < -100.0 ? -100.0 : lp;
                lq = lq < -100.0 ? -100.0 : lq;
                const double w = a.targets[i] == 0.0f ? wneg : 1.0;
                const double den = (1.0 - p) * p;
                const double d = (double)a.lambda * w * (p - y) / (den > 1e-12 ? den : 1e-12) / nfin;      // an element the filter drops: 0
                g = isfinite(w * ((y - 1.0) * lq - y * lp)) ? (float)d : 0.0f;
            }
            a.dprob[i] = g;
        }
        if (t == 0) {
            const float l = a.lambda * (float)mean;
            a.loss[0] = l; a.loss[1] = l;
            for (int b = 0; b < a.B; ++b) a.loss[2 + b] = 0.0f;
            a.img_cnt[0] = cnt;
        }
        return;
    }
    // rank: the AP kernel left loss_b and d loss_b / d prob; :1119 (one ranking) or :1121-1131 (the mean over the counted images)
    float unweighted = 0.0f;
    if (a.mode == 1) unweighted = fg_total > 0 ? a.ap_loss[0] : 0.0f;
    else {
        for (int b = 0; b < a.B; ++b) if (a.fg_counts[b] > 0) unweighted += a.ap_loss[b];                  // fp32, image order (:1128)
        if (cnt > 0) unweighted /= (float)cnt;                                                             // :1129-1130
    }
    const float coef = a.mode == 1 ? (fg_total > 0 ? a.lambda : 0.0f) : (cnt > 0 ? a.lambda / (float)cnt : 0.0f);
    for (int i = t; i < total; i += AN_THREADS) {
        const int b = i / a.K, k = i - b * a.K;
        const bool live = k < min(max(a.sel_counts[b], 0), a.K) && (a.mode == 1 || a.fg_counts[b] > 0);
        a.dprob[i] = live ? a.ap_grad[i] * coef : 0.0f;
    }
    if (t == 0) {
        const float l = a.lambda * unweighted;                                                             // :1137
        a.loss[0] = l; a.loss[1] = l;
        for (int b = 0; b < a.B; ++b) a.loss[2 + b] = a.mode == 1 ? 0.0f : (a.fg_counts[b] > 0 ? a.ap_loss[b] : 0.0f);
        a.img_cnt[0] = cnt;
    }
}

struct ScatterArgs {
    const int64_t* sel_index;    // [B][K]
    const int32_t* sel_counts;   // [B]
    const float* dscore;         // [B][K] d loss / d (score that went into the layer)
    const float* acceptance;     // [B][R] or null
    const float* prob;           // [B][R][C] or null: the scores read max(prob[1:])
    const int32_t* cls_pred;     // [B][R]: arg max over prob[1:], + 1 (gnms_detect3d_scores); with prob
    int B, K, R, C;
    float* dacc;                 // [B][R] or null
    float* dprob;                // [B][R][C] or null
};

__global__ __launch_bounds__(AN_THREADS) void after_nms_scatter_kernel(ScatterArgs a) {
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * AN_THREADS;
    const int rows = min(AN_THREADS, a.R - r0);
    const long long row0 = (long long)b * a.R + r0;
    if (a.dacc && (int)threadIdx.x < rows) a.dacc[row0 + threadIdx.x] = 0.0f;
    if (a.dprob) {
        float* z = a.dprob + row0 * a.C;
        for (int i = threadIdx.x; i < rows * a.C; i += AN_THREADS) z[i] = 0.0f;
    }
    __syncthreads();
    const int cnt = min(max(a.sel_counts[b], 0), a.K);
    for (int k = threadIdx.x; k < cnt; k += AN_THREADS) {
        const long long r = (long long)a.sel_index[(long long)b * a.K + k];
        if (r < r0 || r >= r0 + rows) continue;
        const long long row = (long long)b * a.R + r;
        const float g = a.dscore[(long long)b * a.K + k];
        if (a.prob) {
            int c = a.cls_pred[row];
            c = c < 1 ? 1 : (c >= a.C ? a.C - 1 : c);
            if (a.dacc) a.dacc[row] = g * a.prob[row * a.C + c];
            a.dprob[row * a.C + c] = a.acceptance ? g * a.acceptance[row] : g;
        } else if (a.dacc) {
            a.dacc[row] = g;
        }
    }
}

}  // namespace

extern "C" int gnms_after_nms_decode(const int64_t* sel_index, const int32_t* sel_counts, int B, int K, int R, const float* bbox_2d,
                                     const float* bbox_3d, int D3, const float* raw_gt, int64_t ld_raw_gt, const float* rois, int ld_rois,
                                     const float* rois_3d, int ld_rois_3d, const float* rois_3d_cen, const double* p2, int p2_rows,
                                     const double* scale_factor, const double* means_host, const double* stds_host, const double* gts_val,
                                     const double* gts_3d, int ld_gts_3d, int M, const int32_t* val_counts, float* boxes2d, float* cuboids,
                                     float* gt_params, float* gt_boxes, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && K >= 1 && R >= 1 && M >= 1, "gnms_after_nms_decode: B >= 0, K >= 1, R >= 1, M >= 1 (got %d, %d, %d, %d)", B, K, R, M);
    GNMS_CHECK_ARG(D3 >= 10 && ld_raw_gt >= 21 && ld_rois >= 4 && ld_rois_3d >= 11 && ld_gts_3d >= 11 && (p2_rows == 3 || p2_rows == 4),
                   "gnms_after_nms_decode: bbox_3d >= 10, raw_gt >= 21, rois >= 4, rois_3d >= 11, gts_3d >= 11 columns, p2 of 3 or 4 rows");
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(B <= 65535, "gnms_after_nms_decode: B=%d exceeds 65535", B);
    GNMS_CHECK_ARG(sel_index && sel_counts && bbox_2d && bbox_3d && raw_gt && rois && rois_3d && rois_3d_cen && p2 && scale_factor && means_host &&
                   stds_host && gts_val && gts_3d && val_counts && boxes2d && cuboids && gt_params && gt_boxes, "gnms_after_nms_decode: null pointer");
    DecodeArgs a;
    a.sel_index = sel_index; a.sel_counts = sel_counts; a.b2 = bbox_2d; a.b3 = bbox_3d; a.gt = raw_gt; a.rois = rois; a.r3 = rois_3d;
    a.cen = rois_3d_cen; a.p2 = p2; a.scale = scale_factor; a.gts_val = gts_val; a.gts_3d = gts_3d; a.val_counts = val_counts;
    a.ld_b3 = D3; a.ld_rois = ld_rois; a.ld_r3 = ld_rois_3d; a.p2_rows = p2_rows; a.ld_g3 = ld_gts_3d; a.ld_gt = ld_raw_gt;
    a.B = B; a.K = K; a.R = R; a.M = M;
    for (int i = 0; i < 13; ++i) { a.means[i] = (float)means_host[i]; a.stds[i] = (float)stds_host[i]; }
    a.boxes = boxes2d; a.cuboids = cuboids; a.gt_params = gt_params; a.gt_boxes = gt_boxes;
    after_nms_decode_kernel<<<dim3(gnms_div_up(K > M ? K : M, AN_THREADS), B), AN_THREADS, 0, (hipStream_t)stream>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_after_nms_finish(int phase, int mode, int B, int K, const int32_t* fg_counts, const int32_t* sel_counts, const float* prob,
                                     float* targets, const float* ap_loss, const float* ap_grad, float after_nms_lambda,
                                     int32_t* tail_counts, float* targets_padded, float* loss, int32_t* img_cnt, float* dprob,
                                     const int64_t* best_index, int M, void* stream) {
    GNMS_CHECK_ARG((phase == 0 || phase == 1) && mode >= 0 && mode <= 2, "gnms_after_nms_finish: phase 0 or 1, mode 0 (rank), 1 (rank, all images at once) or 2 (classify)");
    GNMS_CHECK_ARG(B >= 0 && K >= 1, "gnms_after_nms_finish: B >= 0 and K >= 1 (got %d, %d)", B, K);
    GNMS_CHECK_ARG((long long)B * K <= 2147483647LL, "gnms_after_nms_finish: B * K exceeds int32");
    GNMS_CHECK_ARG(fg_counts || B == 0, "gnms_after_nms_finish: null pointer");
    if (phase == 0) GNMS_CHECK_ARG(B == 0 || (sel_counts && targets && tail_counts && targets_padded && best_index && M >= 1),
                                   "gnms_after_nms_finish: phase 0 null pointer or M < 1");
    else GNMS_CHECK_ARG(loss && img_cnt && (B == 0 || (sel_counts && dprob && (mode == 2 ? (prob && targets) : (ap_loss && ap_grad)))),
                        "gnms_after_nms_finish: phase 1 null pointer");
    FinishArgs a;
    a.phase = phase; a.mode = mode; a.B = B; a.K = K; a.fg_counts = fg_counts; a.sel_counts = sel_counts; a.prob = prob; a.targets = targets; a.best_index = best_index; a.M = M;
    a.ap_loss = ap_loss; a.ap_grad = ap_grad; a.lambda = after_nms_lambda; a.tail_counts = tail_counts; a.targets_padded = targets_padded;
    a.loss = loss; a.img_cnt = img_cnt; a.dprob = dprob;
    if (B == 0 && phase == 0) return GNMS_OK;
    after_nms_finish_kernel<<<1, AN_THREADS, 0, (hipStream_t)stream>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_after_nms_scatter(const int64_t* sel_index, const int32_t* sel_counts, const float* dscore, int B, int K, int R, int C,
                                      const float* acceptance, const float* prob, const int32_t* cls_pred, float* dacceptance, float* dprob,
                                      void* stream) {
    GNMS_CHECK_ARG(B >= 0 && K >= 1 && R >= 1, "gnms_after_nms_scatter: B >= 0, K >= 1, R >= 1 (got %d, %d, %d)", B, K, R);
    GNMS_CHECK_ARG((prob != nullptr) == (dprob != nullptr) && (prob == nullptr || (cls_pred != nullptr && C >= 2)),
                   "gnms_after_nms_scatter: prob, cls_pred (C >= 2) and dprob go together");
    GNMS_CHECK_ARG((acceptance != nullptr) == (dacceptance != nullptr) && (acceptance || prob), "gnms_after_nms_scatter: acceptance and dacceptance go together, and one head must be given");
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(B <= 65535, "gnms_after_nms_scatter: B=%d exceeds 65535", B);
    GNMS_CHECK_ARG(sel_index && sel_counts && dscore, "gnms_after_nms_scatter: null pointer");
    ScatterArgs a;
    a.sel_index = sel_index; a.sel_counts = sel_counts; a.dscore = dscore; a.acceptance = acceptance; a.prob = prob; a.cls_pred = cls_pred;
    a.B = B; a.K = K; a.R = R; a.C = C; a.dacc = dacceptance; a.dprob = dprob;
    after_nms_scatter_kernel<<<dim3(gnms_div_up(R, AN_THREADS), B), AN_THREADS, 0, (hipStream_t)stream>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
