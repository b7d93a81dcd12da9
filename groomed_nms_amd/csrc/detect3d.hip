// detect3d.hip -- the inference post-processing of the detection head on the device: everything lib/rpn_util.py::im_detect_3d does
// between `net(im)` and the returned `aboxes` (:1087-1356), around the NMS routes this library already has.
//
//   gnms_detect3d_scores    :1193-1194, :1253-1256   class argmax / max over prob[:, 1:], times the acceptance probability -- the ONLY
//                                                    pass over all A anchors (reads C floats [+ 1], writes a score and a class)
//   gnms_detect3d_decode    :1111-1170, :1182-1215   for the K anchors the top-K selected: 2D box (bbox_decode.h, shared with
//                                                    gnms_bbox_transform_inv), the 3D head de-normalised and applied to the anchor priors,
//                                                    and -- on request -- the camera-space cuboid the 3D overlaps read (float64)
//   gnms_detect3d_assemble  :1338-1351               the kept rows x1 y1 x2 y2 score cls coords_3d[7] tracker, optionally clipped
//
// The reference decodes every anchor on the device, copies ~25 floats per anchor to the host, sorts there and keeps 3000, then 500
// (97.6 % of the decode is thrown away).  Here the selection comes first (gnms_select_topk on the scores), and the full-width head rows
// are gathered for the selected anchors only.  One lane per box, per-image constants (p2_inv, scale factor, clip bounds) are indexed by
// blockIdx.y and so become uniform loads; the normalisation columns travel as kernel arguments.  No allocation, no synchronisation:
// every entry is stream-ordered and can be captured into a graph.
#include "gnms_common.h"
#include "bbox_decode.h"

namespace {

constexpr int kNormCols = 13;                       // bbox_means / bbox_stds: 4 (2D) + 9 (x y z w h l ry sin cos)
struct NormCols { float mean[kNormCols]; float stdv[kNormCols]; };

// np.argmax / np.amax over p[1..C): first maximum on ties; a NaN is the maximum (the first one), as NumPy has it
template <bool VEC4>
__global__ __launch_bounds__(256) void detect3d_scores_kernel(const float* __restrict__ prob, const float* __restrict__ acceptance, long acc_ld,
                                                              int A, int C, float* __restrict__ scores, int* __restrict__ cls_pred) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= A) return;
    const size_t row = (size_t)b * A + i;
    float best;
    int idx = 1;
    if (VEC4) {                                                         // C == 4: one 16-byte load per anchor
        const float4 p = reinterpret_cast<const float4*>(prob)[row];
        best = p.y;
        if (p.z > best || (p.z != p.z && best == best)) { best = p.z; idx = 2; }
        if (p.w > best || (p.w != p.w && best == best)) { best = p.w; idx = 3; }
    } else {
        const float* p = prob + row * C;
        best = p[1];
        for (int c = 2; c < C; ++c) {
            const float v = p[c];
            if (v > best || (v != v && best == best)) { best = v; idx = c; }
        }
    }
    if (acceptance) best = best * acceptance[row * acc_ld];             // :1256, one fp32 product
    scores[row] = best;
    cls_pred[row] = idx;
}

__device__ __forceinline__ long clamp_index(long a, long n) { return a < 0 ? 0 : (a >= n ? n - 1 : a); }

template <bool DECOMP>
__global__ __launch_bounds__(256) void detect3d_decode_kernel(const long long* __restrict__ sel_index, long ld_index, const int* __restrict__ counts,
                                                              int K, int A, const float4* __restrict__ bbox_2d, const float* __restrict__ bbox_3d,
                                                              int D3, const float* __restrict__ rois, const float* __restrict__ anchors,
                                                              int n_anchors, int cols, NormCols nm, const double* __restrict__ p2_inv,
                                                              const float* __restrict__ scale, float4* __restrict__ boxes2d,
                                                              float* __restrict__ coords, float* __restrict__ raw) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= K) return;
    const size_t o = (size_t)b * K + k;
    if (k >= gnms_count(counts, b, K)) {                                // padding behind the image's count
        if (boxes2d) boxes2d[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < 7; ++c) {
            if (coords) coords[o * 7 + c] = 0.f;
            if (raw) raw[o * 7 + c] = 0.f;
        }
        return;
    }
    const long a = clamp_index(sel_index[(size_t)b * ld_index + k], A);  // (a bad index must not read out of bounds)
    const float sf = scale ? scale[b] : 1.0f;
    const float* r = rois + a * 5;
    const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    if (boxes2d) {                                                      // :1182 bbox_transform_inv, :1190 /= scale_factor
        float4 bx = gnms_bbox_decode(make_float4(r0, r1, r2, r3), bbox_2d[(size_t)b * A + a], make_float4(nm.mean[0], nm.mean[1], nm.mean[2], nm.mean[3]),
                                     make_float4(nm.stdv[0], nm.stdv[1], nm.stdv[2], nm.stdv[3]), 1, 1);
        bx.x /= sf; bx.y /= sf; bx.z /= sf; bx.w /= sf;
        boxes2d[o] = bx;
    }
    if (!coords && !raw) return;
    const float* h = bbox_3d + ((size_t)b * A + a) * D3;
    const float* src = anchors + clamp_index((long)r[4], n_anchors) * cols + 4;   // :1131-1132 anchors[tracker, 4:]
    float x = h[0] * nm.stdv[4] + nm.mean[4];                           // :1123-1128
    float y = h[1] * nm.stdv[5] + nm.mean[5];
    float z = h[2] * nm.stdv[6] + nm.mean[6];
    float w = h[3] * nm.stdv[7] + nm.mean[7];
    float hh = h[4] * nm.stdv[8] + nm.mean[8];
    float l = h[5] * nm.stdv[9] + nm.mean[9];
    const float widths = r2 - r0 + 1.0f;                                // :1135-1138
    const float heights = r3 - r1 + 1.0f;
    const float ctr_x = r0 + 0.5f * widths;
    const float ctr_y = r1 + 0.5f * heights;
    x = x * widths + ctr_x;                                             // :1140-1141
    y = y * heights + ctr_y;
    z = src[0] + z;                                                     // :1143
    w = expf(w) * src[1];                                               // :1144-1146
    hh = expf(hh) * src[2];
    l = expf(l) * src[3];
    float ry;
    if (DECOMP) {
        float rsin = h[6] * nm.stdv[11] + nm.mean[11];                  // :1111-1112
        float rcos = h[7] * nm.stdv[12] + nm.mean[12];
        rsin = src[5] + rsin;                                           // :1158-1159
        rcos = src[6] + rcos;
        ry = rcos;                                                      // :1163-1165
        if (h[8] >= 0.5f) ry = rsin;
        if (h[9] >= 0.5f) ry = ry + 3.14159265358979323846f;
    } else {
        ry = (h[6] * nm.stdv[10] + nm.mean[10]) + src[4];               // :1120, :1167
    }
    x /= sf;                                                            // :1191
    y /= sf;
    if (coords) {
        float* c = coords + o * 7;
        c[0] = x; c[1] = y; c[2] = z; c[3] = w; c[4] = hh; c[5] = l; c[6] = ry;
    }
    if (raw) {                                                          // :1205-1215, float64 like the NumPy half of the reference
        const double* P = p2_inv + (size_t)b * 16;
        const double X = (double)(x * z), Y = (double)(y * z), Z = (double)z;   // (the products are fp32 there, :1205)
        const double x3 = P[0] * X + P[1] * Y + P[2] * Z + P[3];
        const double y3 = P[4] * X + P[5] * Y + P[6] * Z + P[7];
        const double z3 = P[8] * X + P[9] * Y + P[10] * Z + P[11];
        const double pi = 3.14159265358979323846;
        double ry3 = (double)ry + atan2(-z3, x3) + 0.5 * pi;            // lib/util.py:641-644
        for (int it = 0; it < 64 && ry3 > pi; ++it) ry3 -= pi * 2;       // (bounded: an infinite angle must not spin for ever)
        for (int it = 0; it < 64 && ry3 <= -pi; ++it) ry3 += pi * 2;
        float* c = raw + o * 7;
        c[0] = (float)x3; c[1] = (float)y3; c[2] = (float)z3; c[3] = w; c[4] = hh; c[5] = l; c[6] = (float)ry3;
    }
}

__device__ __forceinline__ float clipf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // np.clip: NaN stays NaN

template <typename KeepT>
__global__ __launch_bounds__(256) void detect3d_assemble_kernel(const KeepT* __restrict__ keep, long ld_keep, const int* __restrict__ keep_counts,
                                                                const float* __restrict__ sel_scores, long ld_scores,
                                                                const long long* __restrict__ sel_index, long ld_index,
                                                                const int* __restrict__ cls_pred, const float4* __restrict__ boxes2d,
                                                                const float* __restrict__ coords, const float* __restrict__ rois, int K, int A,
                                                                const float* __restrict__ clip_hw, float* __restrict__ out,
                                                                int* __restrict__ out_counts) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= K) return;
    const int n = gnms_count(keep_counts, b, K);
    if (j == 0 && out_counts) out_counts[b] = n;
    float* row = out + ((size_t)b * K + j) * 14;
    const long k = j < n ? (keep ? (long)keep[(size_t)b * ld_keep + j] : (long)j) : -1;
    if (k < 0 || k >= K) {                                              // padding (and an index no NMS route can produce)
        for (int c = 0; c < 14; ++c) row[c] = 0.f;
        return;
    }
    const long a = clamp_index(sel_index[(size_t)b * ld_index + k], A);
    float4 bx = boxes2d[(size_t)b * K + k];
    if (clip_hw) {                                                      // :1347-1351
        const float hi_y = clip_hw[2 * b] - 1.0f, hi_x = clip_hw[2 * b + 1] - 1.0f;
        bx.x = clipf(bx.x, 0.f, hi_x); bx.y = clipf(bx.y, 0.f, hi_y); bx.z = clipf(bx.z, 0.f, hi_x); bx.w = clipf(bx.w, 0.f, hi_y);
    }
    row[0] = bx.x; row[1] = bx.y; row[2] = bx.z; row[3] = bx.w;
    row[4] = sel_scores[(size_t)b * ld_scores + k];
    row[5] = (float)cls_pred[(size_t)b * A + a];
    const float* c3 = coords + ((size_t)b * K + k) * 7;
    for (int c = 0; c < 7; ++c) row[6 + c] = c3[c];
    row[13] = (float)(long)rois[a * 5 + 4];                             // tracker (:1131)
}

}  // namespace

extern "C" int gnms_detect3d_scores(const float* prob, const float* acceptance, int64_t acceptance_ld, int B, int A, int C, float* scores,
                                    int32_t* cls_pred, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && A >= 0, "gnms_detect3d_scores: negative size");
    GNMS_CHECK_ARG(C >= 2, "gnms_detect3d_scores: prob needs a background column and at least one class (C=%d)", C);
    GNMS_CHECK_ARG(!acceptance || acceptance_ld >= 1, "gnms_detect3d_scores: acceptance_ld must be >= 1");
    if (B == 0 || A == 0) return GNMS_OK;
    GNMS_CHECK_ARG(prob && scores && cls_pred, "gnms_detect3d_scores: null pointer");
    GNMS_CHECK_ARG(B <= 65535, "gnms_detect3d_scores: B=%d exceeds 65535", B);
    const dim3 grid((unsigned)gnms_div_up(A, 256), (unsigned)B);
    if (C == 4 && (uintptr_t)prob % 16 == 0)
        detect3d_scores_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(prob, acceptance, (long)acceptance_ld, A, C, scores, cls_pred);
    else
        detect3d_scores_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(prob, acceptance, (long)acceptance_ld, A, C, scores, cls_pred);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_detect3d_decode(const int64_t* sel_index, int64_t ld_index, const int32_t* counts, int B, int K, int A, const float* bbox_2d,
                                    const float* bbox_3d, int D3, const float* rois, const float* anchors, int n_anchors, int anchor_cols,
                                    const float* means_host, const float* stds_host, int norm_cols, int decomp_alpha, const double* p2_inv,
                                    const float* scale_factor, float* boxes2d, float* coords_3d, float* coords_3d_raw, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && K >= 0 && A >= 0, "gnms_detect3d_decode: negative size");
    if (B == 0 || K == 0) return GNMS_OK;
    GNMS_CHECK_ARG(A > 0, "gnms_detect3d_decode: K=%d boxes selected among no anchors", K);
    GNMS_CHECK_ARG(B <= 65535, "gnms_detect3d_decode: B=%d exceeds 65535", B);
    GNMS_CHECK_ARG(sel_index && rois && ld_index >= K, "gnms_detect3d_decode: sel_index / rois missing or ld_index < K");
    GNMS_CHECK_ARG(means_host && stds_host, "gnms_detect3d_decode: bbox_means / bbox_stds missing");
    const bool want3d = coords_3d || coords_3d_raw;
    const int need_norm = want3d ? (decomp_alpha ? 13 : 11) : 4;
    GNMS_CHECK_ARG(norm_cols >= need_norm && need_norm <= kNormCols, "gnms_detect3d_decode: bbox_means / bbox_stds have %d columns, %d needed", norm_cols, need_norm);
    if (boxes2d) {
        GNMS_CHECK_ARG(bbox_2d != nullptr, "gnms_detect3d_decode: boxes2d needs bbox_2d");
        GNMS_CHECK_ARG(((uintptr_t)bbox_2d % 16 == 0) && ((uintptr_t)boxes2d % 16 == 0), "gnms_detect3d_decode: bbox_2d / boxes2d must be 16-byte aligned");
    }
    if (want3d) {
        GNMS_CHECK_ARG(bbox_3d && anchors && n_anchors > 0, "gnms_detect3d_decode: the 3D outputs need bbox_3d and the anchor table");
        GNMS_CHECK_ARG(D3 >= (decomp_alpha ? 10 : 7), "gnms_detect3d_decode: bbox_3d has %d columns, %d needed", D3, decomp_alpha ? 10 : 7);
        GNMS_CHECK_ARG(anchor_cols >= (decomp_alpha ? 11 : 9), "gnms_detect3d_decode: the anchor table has %d columns, %d needed", anchor_cols, decomp_alpha ? 11 : 9);
        GNMS_CHECK_ARG(!coords_3d_raw || p2_inv, "gnms_detect3d_decode: coords_3d_raw needs p2_inv");
    }
    NormCols nm;
    for (int c = 0; c < kNormCols; ++c) {
        nm.mean[c] = c < norm_cols ? means_host[c] : 0.f;
        nm.stdv[c] = c < norm_cols ? stds_host[c] : 1.f;
    }
    const dim3 grid((unsigned)gnms_div_up(K, 256), (unsigned)B);
#define GNMS_DECODE(DEC)                                                                                                                     \
    detect3d_decode_kernel<DEC><<<grid, 256, 0, (hipStream_t)stream>>>((const long long*)sel_index, (long)ld_index, counts, K, A,            \
                                                                       reinterpret_cast<const float4*>(bbox_2d), bbox_3d, D3, rois, anchors,     \
                                                                       n_anchors, anchor_cols, nm, p2_inv, scale_factor,                         \
                                                                       reinterpret_cast<float4*>(boxes2d), coords_3d, coords_3d_raw)
    if (decomp_alpha) GNMS_DECODE(true); else GNMS_DECODE(false);
#undef GNMS_DECODE
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_detect3d_assemble(const void* keep, int keep_is_i64, int64_t ld_keep, const int32_t* keep_counts, const float* sel_scores,
                                      int64_t ld_scores, const int64_t* sel_index, int64_t ld_index, const int32_t* cls_pred,
                                      const float* boxes2d, const float* coords_3d, const float* rois, int B, int K, int A,
                                      const float* clip_hw, float* out, int32_t* out_counts, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && K >= 0 && A >= 0, "gnms_detect3d_assemble: negative size");
    if (B == 0) return GNMS_OK;
    if (K == 0) {
        if (out_counts) GNMS_CHECK_HIP(hipMemsetAsync(out_counts, 0, sizeof(int32_t) * B, (hipStream_t)stream));
        return GNMS_OK;
    }
    GNMS_CHECK_ARG(A > 0, "gnms_detect3d_assemble: K=%d boxes among no anchors", K);
    GNMS_CHECK_ARG(B <= 65535, "gnms_detect3d_assemble: B=%d exceeds 65535", B);
    GNMS_CHECK_ARG(sel_scores && sel_index && cls_pred && boxes2d && coords_3d && rois && out, "gnms_detect3d_assemble: null pointer");
    GNMS_CHECK_ARG(ld_scores >= K && ld_index >= K && (!keep || ld_keep >= K), "gnms_detect3d_assemble: a leading dimension is smaller than K");
    GNMS_CHECK_ARG((uintptr_t)boxes2d % 16 == 0, "gnms_detect3d_assemble: boxes2d must be 16-byte aligned");
    const dim3 grid((unsigned)gnms_div_up(K, 256), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (keep && !keep_is_i64)
        detect3d_assemble_kernel<int><<<grid, 256, 0, st>>>((const int*)keep, (long)ld_keep, keep_counts, sel_scores, (long)ld_scores,
                                                            (const long long*)sel_index, (long)ld_index, cls_pred, reinterpret_cast<const float4*>(boxes2d),
                                                            coords_3d, rois, K, A, clip_hw, out, out_counts);
    else
        detect3d_assemble_kernel<long long><<<grid, 256, 0, st>>>((const long long*)keep, (long)ld_keep, keep_counts, sel_scores, (long)ld_scores,
                                                                  (const long long*)sel_index, (long)ld_index, cls_pred,
                                                                  reinterpret_cast<const float4*>(boxes2d), coords_3d, rois, K, A, clip_hw, out, out_counts);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
