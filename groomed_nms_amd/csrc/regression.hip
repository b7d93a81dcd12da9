// regression.hip -- what the reference's RPN loss does with the sampled foreground (lib/loss/rpn_3d.py:1154-1407, fed by :206-233,
// :316-363, :477-579, :617-621): the 2D and 3D smooth-L1 terms with the sin / cos choice, the axis and head cross entropies, the
// -log IoU term, the acceptance-probability weighting, the uncertainty term with its running weight, the statistics, and the gradients
// of the three heads.  DESIGN.md 3.15.
//
// gnms_reg_loss: two stream-ordered launches over the grid (ceil(R / 256), B), no global atomics, no workgroup waits for another, no
// allocation, nothing read back.  The active anchors of image b are fg_index[b][0 .. fg_counts[b]) (gnms_sample_anchors); workgroup
// (w, b) owns entries w * 256 .. w * 256 + 255 of that list, one lane per active anchor.
//   reg_loss_terms   zeroes the gradient rows of anchors w * 256 .. of image b (every element of the dense gradients is written),
//                    then gathers its lanes' rows, evaluates every term once (eval_anchor) and leaves the workgroup's sums (float64
//                    butterflies over the wave, then the four waves in order) and counts (one ballot each)
//                    -- unweighted and acceptance-weighted, because which of the two the loss uses is only known once the running
//                    weight is -- in its slot of the workspace with plain stores.  A workgroup behind the image's count writes no slot.
//   reg_loss_finish  every workgroup that owns active anchors sums the live slots in the same fixed order (so all of them, and every
//                    run, get the same bits), derives the divisors, the running weight and the weighting decision (:1323-1344),
//                    evaluates its anchors again and scatters their gradient rows; workgroup (0, 0) writes the loss, the statistics
//                    and un_state.  The old un_state is read from a copy that reg_loss_terms left in the workspace, so no workgroup
//                    reads what workgroup (0, 0) is writing.
// The per-anchor arithmetic is float64 on the float32 inputs: a few thousand anchors of latency-bound work, where the wider format
// costs nothing that shows and the result is nearer to the exact value than the reference's float32 chain is.  A term counts as
// finite (:1324-1334, :1358-1364, :1392, :1400) when its float64 value is.
#include <math.h>
#include "gnms_common.h"

namespace {

constexpr int REG_THREADS = 256;
constexpr int REG_WAVES = REG_THREADS / GNMS_WAVE;
constexpr int REG_PARTS = 4;                     // reg_loss_finish: slots j = p, p + 4, ... are summed by part p, then the parts in order
constexpr int REG_SLOT = 64;                     // doubles per slot
constexpr int REG_SNAP_TRIPS = 1024;             // trip bound of the snap_to_pi loops (csrc/kitti_rows.hip)
constexpr double REG_PI = 3.141592653589793;     // math.pi

// a slot's entries (counts are kept as doubles: exact below 2^53)
enum {
    Q_N = 0,          // active anchors
    Q_S2D = 1,        // 4: sums of the 2D smooth-L1 terms (plain: a NaN stays, :1182-1185)
    Q_U = 5,          // 7: sums over the finite elements of x, y, z, w, h, l, rot before the acceptance weighting (:1324-1330)
    Q_UC = 12,        // 7: their finite counts
    Q_UAX = 19,       // 2: the same for axis, head (:1333-1334)
    Q_UAXC = 21,      // 2
    Q_W = 23,         // 7: sums over the finite elements after the acceptance weighting (:1345-1351, :1358-1364)
    Q_WC = 30,        // 7
    Q_AXP = 37,       // 2: plain sums of axis, head without the weighting (:1367)
    Q_AXW = 39,       // 2: with it
    Q_ACC = 41,       // sum of the acceptance (:1356)
    Q_ONEM = 42,      // sum of 1 - acceptance (:1377)
    Q_CEN = 43, Q_CENM = 44, Q_Z = 45, Q_ROT = 46, Q_AXOK = 47, Q_HDOK = 48,
    Q_IOU = 49,       // sum of the finite IoUs (:1392)
    Q_IOUC = 50,
    Q_IOUNZ = 51,     // IoUs != 0 (:1395; a NaN counts)
    Q_LOG = 52,       // sum of the finite -log IoU (:1396-1400)
    Q_LOGC = 53,
    Q_USED = 54
};
static_assert(Q_USED <= REG_SLOT, "slot too small");

// the entries that count lanes (0 or 1 per lane): a wave sums them with one ballot instead of a float64 butterfly
__host__ __device__ constexpr bool is_count(int k) {
    return k == Q_N || (k >= Q_UC && k < Q_UC + 7) || (k >= Q_UAXC && k < Q_UAXC + 2) || (k >= Q_WC && k < Q_WC + 7) || k == Q_CENM ||
           k == Q_AXOK || k == Q_HDOK || k == Q_IOUC || k == Q_IOUNZ || k == Q_LOGC;
}

struct RegArgs {
    const float* b2;             // [B][R][4]
    const float* b3;             // [B][R][ld_b3]
    const float* acc;            // [B][R] or null
    const float* tr;             // [B][R] rows of ld_tr
    const float* gt;             // [B][R] rows of ld_gt
    const float* rois;           // [B][R] rows of ld_rois
    const float* r3;             // [B][R] rows of ld_r3
    const float* cen;            // [B][R][2]
    const double* p2;            // [B][p2_rows][4]
    const double* scale;         // [B]
    const int32_t* fg_index;     // [B][R]
    const int32_t* fg_counts;    // [B]
    const int32_t* counts;       // [B][6]
    int ld_b3, ld_rois, ld_r3, p2_rows;
    long long ld_tr, ld_gt;
    int B, R, nwg;
    double means[13], stds[13];
    double l2d, l3d, lah, liou, un_static;
    int use_acc, dynamic;
    double* un_state;            // [2] or null
    float* loss;
    double* stats;               // [GNMS_REG_STATS]
    int32_t* stat_counts;        // [GNMS_REG_STAT_COUNTS]
    float* d2;
    float* d3;
    float* dacc;                 // null without acc
    double* slots;               // [B * nwg][REG_SLOT]
    double* state_in;            // [2]: un_state as it was when the call began
};

// everything the loss takes from one active anchor: the terms' values and their derivatives w.r.t. the heads' entries
struct Anchor {
    double a;                    // acceptance (1 without)
    double s2d[4], g2d[4];       // smooth-L1 of the 2D deltas and its derivative
    double s3d[7], g3d[7];       // x, y, z, w, h, l, rot; rot reads column rot_col
    int rot_col;
    double ce[2], gce[2];        // axis, head
    double cen, zerr, rot;
    bool axok, hdok;
    double iou, giou[4];         // the IoU and its derivative w.r.t. bbox_2d[0..3]
};

__device__ __forceinline__ void smooth_l1(double x, double t, double& v, double& g) {
    const double d = x - t, z = fabs(d);
    v = z < 1.0 ? 0.5 * z * z : z - 0.5;
    g = d <= -1.0 ? -1.0 : (d >= 1.0 ? 1.0 : d);
}

// F.binary_cross_entropy: the logs clamped at -100, the derivative's denominator at 1e-12
__device__ __forceinline__ void bce(double p, double y, double& v, double& g) {
    double lp = log(p), lq = log1p(-p);
    lp = lp < -100.0 ? -100.0 : lp;
    lq = lq < -100.0 ? -100.0 : lq;
    v = (y - 1.0) * lq - y * lp;
    const double den = (1.0 - p) * p;
    g = (p - y) / (den > 1e-12 ? den : 1e-12);
}

__device__ __forceinline__ double snap_to_pi(double a) {
    if (!isfinite(a)) return a;          // (the reference's loop never ends here)
    for (int i = 0; i < REG_SNAP_TRIPS && a > REG_PI; ++i) a -= 2.0 * REG_PI;
    for (int i = 0; i < REG_SNAP_TRIPS && a <= -REG_PI; ++i) a += 2.0 * REG_PI;
    return a;
}

// d min(a, b) / da resp. d max(a, b) / da as torch's backward gives them (a tie is shared)
__device__ __forceinline__ double dmin_da(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double dmax_da(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }

// bbox_transform_inv (rpn_util.py:886-934) of one row
__device__ __forceinline__ void decode_2d(const double d[4], const double* mean, const double* std, double w, double h, double cx, double cy,
                                          double box[4], double& pw, double& ph) {
    const double dx = d[0] * std[0] + mean[0], dy = d[1] * std[1] + mean[1], dw = d[2] * std[2] + mean[2], dh = d[3] * std[3] + mean[3];
    const double px = dx * w + cx, py = dy * h + cy;
    pw = exp(dw) * w;
    ph = exp(dh) * h;
    box[0] = px - 0.5 * pw; box[1] = py - 0.5 * ph; box[2] = px + 0.5 * pw - 1.0; box[3] = py + 0.5 * ph - 1.0;
}

__device__ void eval_anchor(const RegArgs& a, int b, int r, Anchor& o) {
    const long long row = (long long)b * a.R + r;
    const float* b2 = a.b2 + row * 4;
    const float* b3 = a.b3 + row * a.ld_b3;
    const float* tr = a.tr + row * a.ld_tr;
    const float* gt = a.gt + row * a.ld_gt;
    const float* roi = a.rois + row * a.ld_rois;
    const float* r3 = a.r3 + row * a.ld_r3;
    o.a = a.acc ? (double)a.acc[row] : 1.0;
    double p2d[4], t2d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p2d[k] = (double)b2[k];
        t2d[k] = (double)tr[k];
        smooth_l1(p2d[k], t2d[k], o.s2d[k], o.g2d[k]);                                   // :1177-1180
    }
    double p3[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) p3[k] = (double)b3[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) smooth_l1(p3[k], (double)tr[5 + k], o.s3d[k], o.g3d[k]);   // :1232-1237
    const double axis_lbl = (double)gt[19], head_lbl = (double)gt[20];
    const bool use_sin = axis_lbl == 1.0;                                                  // :1273, :1286-1287
    o.rot_col = use_sin ? 6 : 7;
    smooth_l1(use_sin ? p3[6] : p3[7], (double)(use_sin ? tr[12] : tr[13]), o.s3d[6], o.g3d[6]);
    bce(p3[8], axis_lbl, o.ce[0], o.gce[0]);                                               // :1283-1284
    bce(p3[9], head_lbl, o.ce[1], o.gce[1]);
    o.axok = (p3[8] >= 0.5 ? 1.0 : 0.0) == axis_lbl;                                       // :1292, :1297
    o.hdok = (p3[9] >= 0.5 ? 1.0 : 0.0) == head_lbl;

    // :338-363, :532-577
    const double w = (double)roi[2] - (double)roi[0] + 1.0, h = (double)roi[3] - (double)roi[1] + 1.0;
    const double* P = a.p2 + (long long)b * a.p2_rows * 4;
    const double sc = a.scale[b];
    const double x_dn = (p3[0] * a.stds[4] + a.means[4]) * w + (double)a.cen[row * 2 + 0];
    const double y_dn = (p3[1] * a.stds[5] + a.means[5]) * h + (double)a.cen[row * 2 + 1];
    const double z_dn = (double)r3[4] + (p3[2] * a.stds[6] + a.means[6]);
    const double z_raw = z_dn - P[11];
    const double x_raw = ((z_raw + P[11]) * (x_dn / sc) - P[2] * z_raw - P[3]) / P[0];
    const double y_raw = ((z_raw + P[11]) * (y_dn / sc) - P[6] * z_raw - P[7]) / P[5];
    const double ex = x_raw - (double)gt[12], ey = y_raw - (double)gt[13], ez = z_raw - (double)gt[14];
    o.cen = sqrt(ex * ex + ey * ey + ez * ez);                                             // :1202-1204
    o.zerr = fabs(ez);                                                                     // :576
    double rot = use_sin ? (double)r3[9] + (p3[6] * a.stds[11] + a.means[11]) : (double)r3[10] + (p3[7] * a.stds[12] + a.means[12]);
    if (head_lbl == 1.0) rot += REG_PI;                                                    // :569-571
    o.rot = fabs(snap_to_pi(rot) - (double)gt[11]);                                        // :573, :577

    // :617-621 with core.py:222-240, 522-529; only where the image's quota fg_num is above 0
    o.iou = 0.0;
    o.giou[0] = o.giou[1] = o.giou[2] = o.giou[3] = 0.0;
    if (a.counts[(long long)b * 6 + 2] > 0) {
        const double cx = (double)roi[0] + 0.5 * w, cy = (double)roi[1] + 0.5 * h;
        double A[4], T[4], pw, ph, tw, th;
        decode_2d(p2d, a.means, a.stds, w, h, cx, cy, A, pw, ph);
        decode_2d(t2d, a.means, a.stds, w, h, cx, cy, T, tw, th);
        const double ixr = fmin(A[2], T[2]) - fmax(A[0], T[0]), iyr = fmin(A[3], T[3]) - fmax(A[1], T[1]);
        const double ix = ixr < 0.0 ? 0.0 : ixr, iy = iyr < 0.0 ? 0.0 : iyr;            // torch.clamp(x, 0) (a NaN stays)
        const double inter = ix * iy;
        const double aw = A[2] - A[0], ah = A[3] - A[1];
        const double uni = aw * ah + (T[2] - T[0]) * (T[3] - T[1]) - inter;
        o.iou = inter / uni;
        const double di = (uni + inter) / (uni * uni), da = -inter / (uni * uni);        // d iou / d inter, d iou / d area_a
        const double mx = ixr >= 0.0 ? 1.0 : 0.0, my = iyr >= 0.0 ? 1.0 : 0.0;          // clamp's backward
        const double g_x1 = -di * iy * mx * dmax_da(A[0], T[0]) - da * ah;
        const double g_x2 = di * iy * mx * dmin_da(A[2], T[2]) + da * ah;
        const double g_y1 = -di * ix * my * dmax_da(A[1], T[1]) - da * aw;
        const double g_y2 = di * ix * my * dmin_da(A[3], T[3]) + da * aw;
        o.giou[0] = (g_x1 + g_x2) * w * a.stds[0];
        o.giou[1] = (g_y1 + g_y2) * h * a.stds[1];
        o.giou[2] = 0.5 * (g_x2 - g_x1) * pw * a.stds[2];
        o.giou[3] = 0.5 * (g_y2 - g_y1) * ph * a.stds[3];
    }
}

// the lane's entry of the image's active list, or -1
__device__ __forceinline__ int active_anchor(const RegArgs& a, int b, int cnt) {
    const int i = blockIdx.x * REG_THREADS + threadIdx.x;
    if (i >= cnt) return -1;
    const int r = a.fg_index[(long long)b * a.R + i];
    return (r >= 0 && r < a.R) ? r : -1;
}

__device__ __forceinline__ int image_count(const RegArgs& a, int b) {
    const int c = a.fg_counts[b];
    return c < 0 ? 0 : (c > a.R ? a.R : c);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 1; s < GNMS_WAVE; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

__global__ __launch_bounds__(REG_THREADS) void reg_loss_terms(RegArgs a) {
    __shared__ double red[REG_WAVES][REG_SLOT];
    const int b = blockIdx.y, w = blockIdx.x;
    // the dense gradients of the workgroup's 256 anchors
    {
        const int r0 = w * REG_THREADS;
        const int rows = min(REG_THREADS, a.R - r0);
        const long long row0 = (long long)b * a.R + r0;
        if ((int)threadIdx.x < rows) {
            reinterpret_cast<float4*>(a.d2)[row0 + threadIdx.x] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (a.dacc) a.dacc[row0 + threadIdx.x] = 0.0f;
        }
        // the bbox_3d rows are one contiguous run: scalar stores up to the first 16-byte boundary and behind the last, float4 between
        float* z = a.d3 + row0 * a.ld_b3;
        const int total = rows * a.ld_b3;
        const int head = min(total, (int)(((16u - (unsigned)((uintptr_t)z & 15u)) & 15u) >> 2));
        const int nvec = (total - head) >> 2;
        float4* zv = reinterpret_cast<float4*>(z + head);
        for (int i = threadIdx.x; i < nvec; i += REG_THREADS) zv[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if ((int)threadIdx.x < head) z[threadIdx.x] = 0.0f;
        const int tail = head + (nvec << 2) + threadIdx.x;
        if (tail < total) z[tail] = 0.0f;
    }
    if (w == 0 && b == 0 && threadIdx.x == 0 && a.un_state) { a.state_in[0] = a.un_state[0]; a.state_in[1] = a.un_state[1]; }
    const int cnt = image_count(a, b);
    if (w * REG_THREADS >= cnt) return;                                  // uniform
    const int r = active_anchor(a, b, cnt);
    double q[Q_USED];
#pragma unroll
    for (int k = 0; k < Q_USED; ++k) q[k] = 0.0;
    if (r >= 0) {
        Anchor o;
        eval_anchor(a, b, r, o);
        q[Q_N] = 1.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[Q_S2D + k] = o.s2d[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double u = o.s3d[k], v = o.s3d[k] * o.a;
            if (isfinite(u)) { q[Q_U + k] = u; q[Q_UC + k] = 1.0; }
            if (isfinite(v)) { q[Q_W + k] = v; q[Q_WC + k] = 1.0; }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (isfinite(o.ce[k])) { q[Q_UAX + k] = o.ce[k]; q[Q_UAXC + k] = 1.0; }
            q[Q_AXP + k] = o.ce[k];
            q[Q_AXW + k] = o.ce[k] * o.a;
        }
        q[Q_ACC] = o.a;
        q[Q_ONEM] = 1.0 - o.a;
        q[Q_CEN] = o.cen;
        q[Q_CENM] = o.cen <= 0.2 ? 1.0 : 0.0;                            // :1206
        q[Q_Z] = o.zerr;
        q[Q_ROT] = o.rot;
        q[Q_AXOK] = o.axok ? 1.0 : 0.0;
        q[Q_HDOK] = o.hdok ? 1.0 : 0.0;
        if (isfinite(o.iou)) { q[Q_IOU] = o.iou; q[Q_IOUC] = 1.0; }
        q[Q_IOUNZ] = o.iou != 0.0 ? 1.0 : 0.0;
        const double nl = -log(o.iou);
        if (isfinite(nl)) { q[Q_LOG] = nl; q[Q_LOGC] = 1.0; }
    }
    const int lane = threadIdx.x & (GNMS_WAVE - 1), wave = threadIdx.x / GNMS_WAVE;
#pragma unroll
    for (int k = 0; k < Q_USED; ++k) {
        const double s = is_count(k) ? (double)__popcll(__ballot(q[k] != 0.0)) : wave_sum(q[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < Q_USED) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < REG_WAVES; ++v) s += red[v][threadIdx.x];
        a.slots[((long long)b * a.nwg + w) * REG_SLOT + threadIdx.x] = s;
    }
}

// what reg_loss_finish derives from the batch's sums
struct Derived {
    double n, W, nf;
    bool weighted, has_iou, write_state;
    double c2d, c3[7], cah, cun, ciou;      // d loss / d (an element's term)
    double t2d, t3d, tun, tiou;
};

__device__ void derive(const RegArgs& a, const double* T, Derived& d) {
    d.n = T[Q_N];
    const double n = d.n;
    d.nf = a.un_state ? a.state_in[0] : 0.0;
    d.W = a.dynamic ? a.state_in[1] : a.un_static;
    d.write_state = false;
    d.weighted = a.use_acc != 0;
    d.t2d = d.t3d = d.tun = d.tiou = 0.0;
    d.c2d = d.cah = d.cun = d.ciou = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) d.c3[k] = 0.0;
    d.has_iou = false;
    if (!(n > 0.0)) return;
    if (a.l2d != 0.0) {                                                   // :1163-1191
        d.t2d = (T[Q_S2D] / n + T[Q_S2D + 1] / n + T[Q_S2D + 2] / n + T[Q_S2D + 3] / n) * a.l2d;
        d.c2d = a.l2d / n;
    }
    if (a.l3d != 0.0) {
        if (a.dynamic) {                                                  // :1323-1341
            // the order of :1324-1330: w, h, l, rot, x, y, z
            double init = T[Q_U + 3] / T[Q_UC + 3];
            init += T[Q_U + 4] / T[Q_UC + 4];
            init += T[Q_U + 5] / T[Q_UC + 5];
            init += T[Q_U + 6] / T[Q_UC + 6];
            init += T[Q_U + 0] / T[Q_UC + 0];
            init += T[Q_U + 1] / T[Q_UC + 1];
            init += T[Q_U + 2] / T[Q_UC + 2];
            init *= a.l3d;
            init += (T[Q_UAX] / T[Q_UAXC] + T[Q_UAX + 1] / T[Q_UAXC + 1]) * a.lah;
            if (d.nf == 0.0) {
                d.W = init;
                d.nf = 1.0;
            } else {
                d.nf = fmin(100.0, d.nf + 1.0);
                d.W = init / d.nf + d.W * (d.nf - 1.0) / d.nf;
            }
            d.write_state = true;
            if (d.W > 0.0) d.weighted = true;                             // :1344
        }
        if (!a.acc) d.weighted = false;                                   // (the host requires acc whenever the weighting can be on)
        const int S = d.weighted ? Q_W : Q_U, SC = d.weighted ? Q_WC : Q_UC, AX = d.weighted ? Q_AXW : Q_AXP;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {                                     // :1358-1364
            s += T[S + k] / T[SC + k];
            d.c3[k] = a.l3d / T[SC + k];
        }
        s += (T[AX] / n + T[AX + 1] / n) * a.lah;                         // :1367
        d.t3d = s * a.l3d;                                                // :1369
        d.cah = a.l3d * a.lah / n;
    } else {
        d.weighted = false;
    }
    if (d.W > 0.0 && a.acc) {                                             // :1375-1382
        d.tun = T[Q_ONEM] / n * d.W;
        d.cun = -d.W / n;
    }
    if (a.liou != 0.0 && T[Q_IOUNZ] > 0.0) {                              // :1395-1403
        d.has_iou = true;
        d.tiou = T[Q_LOG] / T[Q_LOGC] * a.liou;
        d.ciou = a.liou / T[Q_LOGC];
    }
}

__global__ __launch_bounds__(REG_THREADS) void reg_loss_finish(RegArgs a) {
    __shared__ double part[REG_PARTS][REG_SLOT];
    __shared__ double T[REG_SLOT];
    const int b = blockIdx.y, w = blockIdx.x;
    const int cnt = image_count(a, b);
    const bool first = w == 0 && b == 0;
    if (w * REG_THREADS >= cnt && !first) return;                         // uniform
    // the live slots of all images, in the order (image, workgroup)
    {
        const int p = threadIdx.x / REG_SLOT, q = threadIdx.x % REG_SLOT;
        double s = 0.0;
        int j = 0;
        for (int bb = 0; bb < a.B; ++bb) {
            const int live = (image_count(a, bb) + REG_THREADS - 1) / REG_THREADS;
            if (q < Q_USED)
                for (int ww = (p - j % REG_PARTS + REG_PARTS) % REG_PARTS; ww < live; ww += REG_PARTS)
                    s += a.slots[((long long)bb * a.nwg + ww) * REG_SLOT + q];
            j += live;
        }
        part[p][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < REG_SLOT) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int p = 1; p < REG_PARTS; ++p) s += part[p][threadIdx.x];
        T[threadIdx.x] = s;
    }
    __syncthreads();
    Derived d;
    derive(a, T, d);
    if (first && threadIdx.x == 0) {
        const double n = d.n;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double* s = a.stats;
        if (n > 0.0) {
            const double total = d.t2d + d.t3d + d.tun + d.tiou;
            a.loss[0] = (float)total;
            s[0] = d.t2d; s[1] = d.t3d; s[2] = d.tun; s[3] = d.tiou;
            s[4] = T[Q_CEN] / n; s[5] = T[Q_CENM] / n; s[6] = T[Q_Z] / n; s[7] = T[Q_ROT] / n;
            s[8] = T[Q_IOU] / T[Q_IOUC];
            s[9] = a.l3d != 0.0 ? T[Q_AXOK] / n : nan;
            s[10] = a.l3d != 0.0 ? T[Q_HDOK] / n : nan;
            s[11] = (a.acc && a.l3d != 0.0) ? T[Q_ACC] / n : nan;             // :1355 lies inside `if self.bbox_3d_lambda`
            s[12] = total;
            if (d.write_state && a.un_state) { a.un_state[0] = d.nf; a.un_state[1] = d.W; }
        } else {                                                          // :1154: nothing of the block runs
            a.loss[0] = 0.0f;
            for (int k = 0; k < 13; ++k) s[k] = nan;
        }
        s[13] = d.W;
        int32_t* c = a.stat_counts;
        c[0] = (int)n;
        for (int k = 0; k < 7; ++k) { c[1 + k] = (int)T[Q_UC + k]; c[10 + k] = (int)T[Q_WC + k]; }
        c[8] = (int)T[Q_UAXC]; c[9] = (int)T[Q_UAXC + 1];
        c[17] = (int)T[Q_IOUC]; c[18] = (int)T[Q_IOUNZ]; c[19] = (int)T[Q_LOGC];
        c[20] = d.weighted ? 1 : 0; c[21] = d.has_iou ? 1 : 0; c[22] = 0; c[23] = 0;
    }
    if (w * REG_THREADS >= cnt) return;
    const int r = active_anchor(a, b, cnt);
    if (r < 0) return;
    Anchor o;
    eval_anchor(a, b, r, o);
    const long long row = (long long)b * a.R + r;
    const double wgt = d.weighted ? o.a : 1.0;
    // bbox_2d: the 2D term and, through the decode, the IoU term.  An element that an isfinite filter dropped gets 0.
    {
        const double nl = -log(o.iou);
        const double gi = (d.has_iou && isfinite(nl)) ? -d.ciou / o.iou : 0.0;
        float4 g;
        g.x = (float)(d.c2d * o.g2d[0] + (gi != 0.0 ? gi * o.giou[0] : 0.0));
        g.y = (float)(d.c2d * o.g2d[1] + (gi != 0.0 ? gi * o.giou[1] : 0.0));
        g.z = (float)(d.c2d * o.g2d[2] + (gi != 0.0 ? gi * o.giou[2] : 0.0));
        g.w = (float)(d.c2d * o.g2d[3] + (gi != 0.0 ? gi * o.giou[3] : 0.0));
        if (d.c2d == 0.0 && gi == 0.0) g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        reinterpret_cast<float4*>(a.d2)[row] = g;
    }
    if (a.l3d != 0.0) {
        float* g3 = a.d3 + row * a.ld_b3;
        double ga = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const bool fin = isfinite(o.s3d[k] * wgt);
            const float g = fin ? (float)(d.c3[k] * wgt * o.g3d[k]) : 0.0f;
            if (k < 6) g3[k] = g;
            else g3[o.rot_col] = g;                                        // (the other of columns 6, 7 keeps its 0)
            if (fin) ga += d.c3[k] * o.s3d[k];
        }
        g3[8] = (float)(d.cah * wgt * o.gce[0]);
        g3[9] = (float)(d.cah * wgt * o.gce[1]);
        ga += d.cah * (o.ce[0] + o.ce[1]);
        if (a.dacc) a.dacc[row] = (float)((d.weighted ? ga : 0.0) + d.cun);
    } else if (a.dacc) {
        a.dacc[row] = (float)d.cun;
    }
}

int reg_nwg(int R) { return (R + REG_THREADS - 1) / REG_THREADS; }

}  // namespace

extern "C" size_t gnms_reg_loss_workspace_bytes(int B, int R) {
    if (B <= 0 || R <= 0) return 0;
    return ((size_t)B * reg_nwg(R) * REG_SLOT + 2) * sizeof(double);
}

extern "C" int gnms_reg_loss(const float* bbox_2d, const float* bbox_3d, int ld_bbox_3d, const float* acceptance, const float* transforms,
                             int64_t ld_transforms, const float* raw_gt, int64_t ld_raw_gt, const float* rois, int ld_rois,
                             const float* rois_3d, int ld_rois_3d, const float* rois_3d_cen, const double* p2, int p2_rows,
                             const double* scale_factor, const int32_t* fg_index, const int32_t* fg_counts, const int32_t* counts, int B,
                             int R, const double* means, const double* stds, double bbox_2d_lambda, double bbox_3d_lambda,
                             double bbox_axis_head_lambda, double iou_2d_lambda, int use_acceptance, double bbox_un_lambda,
                             int bbox_un_dynamic, double* un_state, float* loss, double* stats, int32_t* stat_counts, float* d_bbox_2d,
                             float* d_bbox_3d, float* d_acceptance, void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 1 && B <= 65535, "gnms_reg_loss: B = %d outside [1, 65535]", B);
    GNMS_CHECK_ARG(R >= 1, "gnms_reg_loss: R = %d < 1", R);
    GNMS_CHECK_ARG(ld_bbox_3d >= 10 && ld_bbox_3d <= 4096, "gnms_reg_loss: bbox_3d rows of %d columns, 10 are read", ld_bbox_3d);
    GNMS_CHECK_ARG(R < (1 << 30) && (long long)B * R * ld_bbox_3d < (1ll << 40), "gnms_reg_loss: B = %d, R = %d too large", B, R);
    GNMS_CHECK_ARG(ld_transforms >= 14, "gnms_reg_loss: transforms rows of %lld columns, 14 are read", (long long)ld_transforms);
    GNMS_CHECK_ARG(ld_raw_gt >= 21, "gnms_reg_loss: raw_gt rows of %lld columns, 21 are read", (long long)ld_raw_gt);
    GNMS_CHECK_ARG(ld_rois >= 4 && ld_rois_3d >= 11, "gnms_reg_loss: rois rows of %d (>= 4), rois_3d rows of %d (>= 11) columns", ld_rois,
                   ld_rois_3d);
    GNMS_CHECK_ARG(p2_rows == 3 || p2_rows == 4, "gnms_reg_loss: p2 of %d rows", p2_rows);
    GNMS_CHECK_ARG(means && stds, "gnms_reg_loss: means / stds is NULL");
    GNMS_CHECK_ARG(bbox_2d_lambda == bbox_2d_lambda && bbox_3d_lambda == bbox_3d_lambda && bbox_axis_head_lambda == bbox_axis_head_lambda &&
                   iou_2d_lambda == iou_2d_lambda && bbox_un_lambda == bbox_un_lambda, "gnms_reg_loss: a weight is NaN");
    GNMS_CHECK_ARG(bbox_2d && bbox_3d && transforms && raw_gt && rois && rois_3d && rois_3d_cen && p2 && scale_factor && fg_index &&
                   fg_counts && counts, "gnms_reg_loss: an input is NULL");
    GNMS_CHECK_ARG(loss && stats && stat_counts && d_bbox_2d && d_bbox_3d, "gnms_reg_loss: an output is NULL");
    const bool needs_acc = use_acceptance || bbox_un_dynamic || (!bbox_un_dynamic && bbox_un_lambda > 0.0);
    GNMS_CHECK_ARG(!needs_acc || (acceptance && d_acceptance),
                   "gnms_reg_loss: the acceptance weighting and the uncertainty term need acceptance and d_acceptance");
    GNMS_CHECK_ARG(!acceptance || d_acceptance, "gnms_reg_loss: acceptance without d_acceptance");
    GNMS_CHECK_ARG(!bbox_un_dynamic || un_state, "gnms_reg_loss: bbox_un_dynamic needs un_state");
    const size_t need = gnms_reg_loss_workspace_bytes(B, R);
    if (!workspace || workspace_bytes < need) {
        gnms_set_error("gnms_reg_loss: workspace of %zu bytes, needs %zu", workspace_bytes, need);
        return GNMS_ERR_WORKSPACE;
    }
    GNMS_CHECK_ARG((uintptr_t)workspace % 8 == 0, "gnms_reg_loss: workspace must be 8-byte aligned");
    GNMS_CHECK_ARG((uintptr_t)d_bbox_2d % 16 == 0, "gnms_reg_loss: d_bbox_2d must be 16-byte aligned");

    RegArgs a = {};
    a.b2 = bbox_2d; a.b3 = bbox_3d; a.acc = acceptance; a.tr = transforms; a.gt = raw_gt; a.rois = rois; a.r3 = rois_3d; a.cen = rois_3d_cen;
    a.p2 = p2; a.scale = scale_factor; a.fg_index = fg_index; a.fg_counts = fg_counts; a.counts = counts;
    a.ld_b3 = ld_bbox_3d; a.ld_rois = ld_rois; a.ld_r3 = ld_rois_3d; a.p2_rows = p2_rows; a.ld_tr = ld_transforms; a.ld_gt = ld_raw_gt;
    a.B = B; a.R = R; a.nwg = reg_nwg(R);
    for (int k = 0; k < 13; ++k) { a.means[k] = means[k]; a.stds[k] = stds[k]; }
    a.l2d = bbox_2d_lambda; a.l3d = bbox_3d_lambda; a.lah = bbox_axis_head_lambda; a.liou = iou_2d_lambda; a.un_static = bbox_un_lambda;
    a.use_acc = use_acceptance != 0; a.dynamic = bbox_un_dynamic != 0;
    a.un_state = bbox_un_dynamic ? un_state : nullptr;
    a.loss = loss; a.stats = stats; a.stat_counts = stat_counts; a.d2 = d_bbox_2d; a.d3 = d_bbox_3d; a.dacc = acceptance ? d_acceptance : nullptr;
    a.slots = static_cast<double*>(workspace);
    a.state_in = a.slots + (size_t)B * a.nwg * REG_SLOT;

    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(a.nwg, B);
    reg_loss_terms<<<grid, REG_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    reg_loss_finish<<<grid, REG_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
