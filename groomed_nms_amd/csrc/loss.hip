// loss.hip -- what RPN_3D_loss (lib/loss/rpn_3d.py) does around its terms: the ground truths of a batch, the total with
// the statistics, and the whole backward.
//
//   gnms_gt_filter          :399-419 on the device: determine_ignores (rpn_util.py:937-962) per ground-truth record in float64,
//                           bbXYWH2Coords, and the stable compaction into gts_val / box_lbls / gts_3d / gts_ign with their counts
//   gnms_loss_combine       the terms' device scalars -> the fp32 total in the reference's order of additions and one float64 vector
//                           of statistics in the order of the reference's `stats` list
//   gnms_loss_grad_combine  upstream gradient (a device scalar) times the terms' dense gradients -> the five heads' gradients
//
// One launch each, no workspace, no atomics, nothing filled beforehand, nothing read back: graph-capturable with the terms between them.
#include <limits.h>

#include "gnms_common.h"

namespace {

constexpr int kThreads = 256;                       // gnms_gt_filter: one thread per record, GNMS_LOSS_MAX_GTS of them
constexpr int kRec = GNMS_LOSS_RECORD_COLS;
constexpr int kSegs = 5;                            // cls, prob, bbox_2d, bbox_3d, acceptance
constexpr int kMaxBlocks = 2048;                    // 8 workgroups of 256 on each of the 256 CUs; the loop strides over the rest

// One workgroup per image.  Thread t owns record t: it decides val / ign / rmv, a ballot per wave and the popcount of the lanes below
// give its place within the wave's kept rows, the four waves' totals in LDS the place of the wave.  Placement depends on nothing but
// the input order.  Rows behind a count are written as zeros by the threads that own them.
__global__ __launch_bounds__(kThreads) void gt_filter_kernel(const double* __restrict__ records, const int32_t* __restrict__ counts, int cap,
                                                             double min_gt_vis, double min_gt_h, double max_gt_h, int use_trunc,
                                                             double* __restrict__ gts_val, int32_t* __restrict__ box_lbls,
                                                             double* __restrict__ gts_3d, double* __restrict__ gts_ign,
                                                             int32_t* __restrict__ val_counts, int32_t* __restrict__ ign_counts) {
    __shared__ int s_val[kThreads / GNMS_WAVE], s_ign[kThreads / GNMS_WAVE];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (GNMS_WAVE - 1), wave = t / GNMS_WAVE;
    int n = counts[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    double2 row[kRec / 2] = {};
    bool val = false, keep_ign = false;
    if (t < n) {
        const double2* src = reinterpret_cast<const double2*>(records + ((size_t)b * cap + t) * kRec);
#pragma unroll
        for (int k = 0; k < kRec / 2; ++k) row[k] = src[k];
        const double h = row[1].y, cls = row[10].x, vis = row[11].x, trunc = row[11].y;
        bool ign = row[10].y != 0.0;                                                  // rpn_util.py:948-952, scale_factor = 1
        ign |= vis < min_gt_vis;
        ign |= h < min_gt_h;
        ign |= h > max_gt_h;
        ign |= cls == 0.0;
        if (use_trunc) ign |= trunc > fmax(1.0 - min_gt_vis, 0.0);                    // :954-955
        const bool rmv = cls < 0.0;                                                   // :957
        val = !rmv && !ign;
        keep_ign = !rmv && ign;
    }
    const unsigned long long m_val = __ballot(val), m_ign = __ballot(keep_ign);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) {
        s_val[wave] = __popcll(m_val);
        s_ign[wave] = __popcll(m_ign);
    }
    __syncthreads();
    int off_val = 0, off_ign = 0, n_val = 0, n_ign = 0;
#pragma unroll
    for (int w = 0; w < kThreads / GNMS_WAVE; ++w) {
        if (w < wave) {
            off_val += s_val[w];
            off_ign += s_ign[w];
        }
        n_val += s_val[w];
        n_ign += s_ign[w];
    }
    const size_t img = (size_t)b * cap;
    if (val || keep_ign) {
        const double x = row[0].x, y = row[0].y;
        const double2 lo = make_double2(x, y), hi = make_double2(row[1].x + (x - 1.0), row[1].y + (y - 1.0));   // rpn_util.py:788-789
        if (val) {
            const size_t j = img + off_val + __popcll(m_val & below);
            double2* d = reinterpret_cast<double2*>(gts_val + j * 4);
            d[0] = lo;
            d[1] = hi;
            box_lbls[j] = (int32_t)row[10].x;
            double2* d3 = reinterpret_cast<double2*>(gts_3d + j * 16);
#pragma unroll
            for (int k = 0; k < 8; ++k) d3[k] = row[2 + k];
        } else {
            double2* d = reinterpret_cast<double2*>(gts_ign + (img + off_ign + __popcll(m_ign & below)) * 4);
            d[0] = lo;
            d[1] = hi;
        }
    }
    if (t < cap) {
        const double2 zero = make_double2(0.0, 0.0);
        if (t >= n_val) {
            double2* d = reinterpret_cast<double2*>(gts_val + (img + t) * 4);
            d[0] = zero;
            d[1] = zero;
            box_lbls[img + t] = 0;
            double2* d3 = reinterpret_cast<double2*>(gts_3d + (img + t) * 16);
#pragma unroll
            for (int k = 0; k < 8; ++k) d3[k] = zero;
        }
        if (t >= n_ign) {
            double2* d = reinterpret_cast<double2*>(gts_ign + (img + t) * 4);
            d[0] = zero;
            d[1] = zero;
        }
    }
    if (t == 0) {
        val_counts[b] = n_val;
        ign_counts[b] = n_ign;
    }
}

// One wave; lane k writes entry k of the statistics, lane 0 the total.
__global__ __launch_bounds__(GNMS_WAVE) void loss_combine_kernel(const float* __restrict__ cls_loss, const double* __restrict__ cls_acc,
                                                                 const float* __restrict__ after_loss, const double* __restrict__ reg_stats, const int32_t* __restrict__ reg_counts,
                                                                 float* __restrict__ total, double* __restrict__ stats) {
    const int k = threadIdx.x;
    const float t_cls = cls_loss ? cls_loss[0] : 0.f, t_after = after_loss ? after_loss[0] : 0.f;
    const bool reg = reg_stats && reg_counts[0] > 0;                                  // :1154: no active anchor, no regression block
    // the regression kernel keeps its four terms in float64; each is rounded once, as the reference's fp32 term is, and added in
    // the reference's order: :999, :1138, :1190, :1371, :1380, :1403
    float sum = 0.f;
    sum += t_cls;
    sum += t_after;
    if (reg) {
        sum += (float)reg_stats[0];
        sum += (float)reg_stats[1];
        sum += (float)reg_stats[2];
        sum += (float)reg_stats[3];
    }
    // fg bg cls after | bbox_2d cen cen_lt axis head conf bbox_3d un z rot iou_2d iou_2d_los | total | the uncertainty weight in use
    constexpr int from_reg[GNMS_LOSS_STATS] = {-1, -1, -1, -1, 0, 4, 5, 9, 10, 11, 1, 2, 6, 7, 8, 3, -1, 13};
    if (k < GNMS_LOSS_STATS) {
        double v = 0.0;
        if (k == 0 || k == 1) v = cls_acc ? cls_acc[k] : 0.0;
        else if (k == 2) v = (double)t_cls;
        else if (k == 3) v = after_loss ? (double)after_loss[1] : 0.0;
        else if (k == 16) v = (double)sum;
        else v = reg_stats ? reg_stats[from_reg[k]] : 0.0;
        stats[k] = v;
    }
    if (k == 0) total[0] = sum;
}

struct GradSeg {
    const float* a;                                 // first addend, or NULL: zero
    const float* b;                                 // second addend, or NULL
    float* out;                                     // NULL: the head takes no gradient
    long long n;                                    // floats
};
struct GradSegs { GradSeg s[kSegs]; };

__device__ __forceinline__ float4 scaled(const float4 v, float g) { return make_float4(v.x * g, v.y * g, v.z * g, v.w * g); }

// Every buffer is one run of contiguous floats whatever its row width (4, C, 10 or 11, 1): 16 bytes per lane and instruction, the whole
// grid strides over one buffer after the other, and the at most three floats behind the last full quad of a buffer go one per lane.
__global__ __launch_bounds__(kThreads) void loss_grad_combine_kernel(GradSegs segs, const float* __restrict__ upstream) {
    const float g = upstream[0];
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
#pragma unroll
    for (int k = 0; k < kSegs; ++k) {
        const float* __restrict__ a = segs.s[k].a;
        const float* __restrict__ b = segs.s[k].b;
        float* __restrict__ out = segs.s[k].out;
        const long long n = segs.s[k].n, quads = n >> 2;
        if (!out) continue;
        for (long long i = tid; i < quads; i += stride) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a) {
                v = reinterpret_cast<const float4*>(a)[i];
                if (b) {
                    const float4 w = reinterpret_cast<const float4*>(b)[i];
                    v = make_float4(v.x + w.x, v.y + w.y, v.z + w.z, v.w + w.w);
                }
                v = scaled(v, g);
            }
            reinterpret_cast<float4*>(out)[i] = v;
        }
        const long long i = (quads << 2) + tid;
        if (i < n) {
            float v = 0.f;
            if (a) v = (b ? a[i] + b[i] : a[i]) * g;
            out[i] = v;
        }
    }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int gnms_gt_filter(const double* records, const int32_t* counts, int B, int capacity, double min_gt_vis, double min_gt_h,
                              double max_gt_h, int use_trunc, double* gts_val, int32_t* box_lbls, double* gts_3d, double* gts_ign,
                              int32_t* val_counts, int32_t* ign_counts, void* stream) {
    GNMS_CHECK_ARG(B >= 0, "gnms_gt_filter: B=%d (>= 0)", B);
    if (capacity < 1 || capacity > GNMS_LOSS_MAX_GTS) {
        gnms_set_error("gnms_gt_filter: capacity=%d records per image, 1..%d are supported", capacity, GNMS_LOSS_MAX_GTS);
        return GNMS_ERR_UNSUPPORTED;
    }
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(records && counts, "gnms_gt_filter: records / counts missing");
    GNMS_CHECK_ARG(gts_val && box_lbls && gts_3d && gts_ign && val_counts && ign_counts, "gnms_gt_filter: null output");
    GNMS_CHECK_ARG(aligned16(records) && aligned16(gts_val) && aligned16(gts_3d) && aligned16(gts_ign),
                   "gnms_gt_filter: records, gts_val, gts_3d and gts_ign must be 16-byte aligned");
    gt_filter_kernel<<<(unsigned)B, kThreads, 0, (hipStream_t)stream>>>(records, counts, capacity, min_gt_vis, min_gt_h, max_gt_h, use_trunc,
                                                                        gts_val, box_lbls, gts_3d, gts_ign, val_counts, ign_counts);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_loss_combine(const float* cls_loss, const double* cls_acc, const float* after_loss, const double* reg_stats, const int32_t* reg_counts, float* total, double* stats, void* stream) {
    GNMS_CHECK_ARG(total && stats, "gnms_loss_combine: null output");
    GNMS_CHECK_ARG(!cls_loss == !cls_acc, "gnms_loss_combine: cls_loss and cls_acc come together");
    GNMS_CHECK_ARG(!reg_stats == !reg_counts, "gnms_loss_combine: reg_stats and reg_counts come together");
    loss_combine_kernel<<<1, GNMS_WAVE, 0, (hipStream_t)stream>>>(cls_loss, cls_acc, after_loss, reg_stats, reg_counts, total, stats);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_loss_grad_combine(const float* upstream, long long rows, int C, int D3, const float* dcls, const float* dprob, const float* d2,
                                      const float* d3, const float* da, const float* dacc, float* g_cls, float* g_prob, float* g_bbox_2d,
                                      float* g_bbox_3d, float* g_acceptance, void* stream) {
    GNMS_CHECK_ARG(rows >= 0 && C >= 0 && D3 >= 0, "gnms_loss_grad_combine: rows=%lld C=%d D3=%d (>= 0 each)", rows, C, D3);
    GNMS_CHECK_ARG(rows <= LLONG_MAX / 64 && C <= 64 && D3 <= 64, "gnms_loss_grad_combine: rows=%lld C=%d D3=%d: too many", rows, C, D3);
    if (rows == 0) return GNMS_OK;
    GNMS_CHECK_ARG(upstream != nullptr, "gnms_loss_grad_combine: the upstream gradient is missing");
    GNMS_CHECK_ARG(!(g_cls || g_prob) || C >= 1, "gnms_loss_grad_combine: gradients of cls / prob need C >= 1");
    GNMS_CHECK_ARG(!g_bbox_3d || D3 >= 1, "gnms_loss_grad_combine: a gradient of bbox_3d needs D3 >= 1");
    GradSegs segs;
    segs.s[0] = {dcls, nullptr, g_cls, rows * C};
    segs.s[1] = {dprob, nullptr, g_prob, rows * C};
    segs.s[2] = {d2, nullptr, g_bbox_2d, rows * 4};
    segs.s[3] = {d3, nullptr, g_bbox_3d, rows * D3};
    segs.s[4] = {da ? da : dacc, da ? dacc : nullptr, g_acceptance, rows};
    long long most = 0;
    for (int k = 0; k < kSegs; ++k) {
        const GradSeg& s = segs.s[k];
        if (!s.out) continue;
        GNMS_CHECK_ARG(aligned16(s.a) && aligned16(s.b) && aligned16(s.out), "gnms_loss_grad_combine: buffer %d is not 16-byte aligned", k);
        most = s.n > most ? s.n : most;
    }
    if (most == 0) return GNMS_OK;
    const long long want = ((most + 3) / 4 + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    loss_grad_combine_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(segs, upstream);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
