// kitti_rows.hip -- from the detections of a batch to the rows the KITTI devkit would parse from the reference's result files, on the
// device (gfx950): the validation tail of lib/train_test.py:99-110 -> lib/rpn_util.py:1489-1631 -> fscanf("%lf") without the files.
//
// Per image: the first min(nms_topN_post, count) rows, those whose score (widened to float64) is > score_thres in their order, the
// back-projection and the two angle conversions in float64, every field rounded through its 6-decimal text, and the row appended
// behind the rows already in a caller-owned buffer.  The running end of that buffer lives on the device (state[]), so that batches
// append one after the other in stream order and the host never learns a count.
//
// Launches (stream-ordered, no workgroup waits for another): count (one workgroup per image -> kept[b]), write (one workgroup per image:
// sums kept[0..b), compacts by ballot, converts, stores), commit (one thread: the new running end).  The write kernel only READS the
// running end; the commit kernel is the only writer, one launch later.
//
// The rounding (round6): the text is '{:.6f}'.format(v), the correctly rounded 6-decimal image of the exact binary value, and strtod
// of it is the double nearest to n / 10^6 with n = round-half-even(v * 10^6).  p = v * 1e6 and e = fma(v, 1e6, -p) give v * 10^6 = p + e
// exactly; r = rint(p) is n unless p lies exactly half way between two integers (|p - r| = 0.5, p - r is exact), where the sign of e
// decides (e = 0: the exact tie, which rint has already sent to the even side).  n < 2^53 and 10^6 are exact doubles and the division
// is IEEE-correct, so n / 1e6 is that nearest double.  Exact for finite |v| < 1e9; anything else passes through and is counted.
// No fast-math: the file relies on IEEE multiplication, fma, division and rint.
#include <math.h>

#include "gnms_common.h"

namespace {

constexpr int kThreads = 256;          // 4 waves per image
constexpr int kWaves = kThreads / GNMS_WAVE;
constexpr int kDetCols = 14;
constexpr int kSnapTrips = 1024;       // trip bound of the snap_to_pi loops: angles up to ~6.4e3 rad wrap like the reference's
constexpr double kPi = 3.141592653589793;        // math.pi
constexpr double kTwoPi = 2.0 * kPi;             // math.pi * 2 (exact doubling)
constexpr double kHalfPi = 0.5 * kPi;            // 0.5 * math.pi
constexpr double kRoundLimit = 1e9;

// float('{:.6f}'.format(v)); *outside: v is not finite or |v| >= 1e9 (returned as it is)
__device__ __forceinline__ double round6(double v, int* outside) {
    if (!(fabs(v) < kRoundLimit)) {
        *outside += 1;
        return v;
    }
    const double p = v * 1e6;
    const double e = fma(v, 1e6, -p);
    double n = rint(p);
    const double d = p - n;
    if (d == 0.5 && e > 0.0) n += 1.0;
    else if (d == -0.5 && e < 0.0) n -= 1.0;
    return copysign(n / 1e6, v);                  // -0.000000 parses to -0.0
}

// lib/math_3d.py:497-510 with a trip bound (a NaN ends the loops at once; *stuck: a finite angle the bound left outside (-pi, pi])
__device__ __forceinline__ double snap_to_pi(double a, int* stuck) {
    for (int i = 0; i < kSnapTrips && a > kPi; ++i) a -= kTwoPi;
    for (int i = 0; i < kSnapTrips && a <= -kPi; ++i) a += kTwoPi;
    if (a > kPi || a <= -kPi) *stuck = 1;
    return a;
}

__device__ __forceinline__ int image_rows(const int32_t* __restrict__ counts, int b, int Kmax, int topn) {
    const int c = gnms_count(counts, b, Kmax);
    return c < topn ? c : topn;
}

__device__ __forceinline__ bool kept(const float* __restrict__ det, int64_t row, double score_thres) {
    return (double)det[row * kDetCols + 4] > score_thres;      // strict, in float64 (NaN: dropped)
}

__global__ __launch_bounds__(kThreads) void count_kernel(const float* __restrict__ det, const int32_t* __restrict__ counts, int Kmax, int topn,
                                                          double score_thres, int32_t* __restrict__ kept_out) {
    __shared__ int s_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int m = image_rows(counts, b, Kmax, topn);
    int n = 0;
    for (int k = tid; k < m; k += kThreads) n += kept(det, (int64_t)b * Kmax + k, score_thres) ? 1 : 0;
    if (n) atomicAdd(&s_n, n);
    __syncthreads();
    if (tid == 0) kept_out[b] = s_n;
}

__global__ __launch_bounds__(kThreads) void write_kernel(const float* __restrict__ det, const int32_t* __restrict__ counts,
                                                          const double* __restrict__ p2_inv, int Kmax, int topn, double score_thres,
                                                          const int32_t* __restrict__ class_ids, int n_lbls, const int32_t* __restrict__ kept_in,
                                                          double* __restrict__ rows, int32_t* __restrict__ lbl_index, int64_t capacity,
                                                          int32_t* __restrict__ offsets, int n_offsets, int image_base, long long* state) {
    __shared__ long long s_pre;
    __shared__ int s_wave[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (GNMS_WAVE - 1), wave = tid / GNMS_WAVE;
    if (tid == 0) s_pre = 0;
    __syncthreads();
    long long pre = 0;                                          // rows of the images before this one in the batch
    for (int i = tid; i < b; i += kThreads) pre += kept_in[i];
    if (pre) atomicAdd((unsigned long long*)&s_pre, (unsigned long long)pre);
    __syncthreads();
    const long long base = state[GNMS_KITTI_ROWS_STATE_END] + s_pre;        // read only: the commit kernel moves the end
    const int m = image_rows(counts, b, Kmax, topn);
    const double* P = p2_inv + (size_t)b * 16;
    int done = 0, outside = 0, stuck = 0, bad_class = 0;
    for (int k0 = 0; k0 < m; k0 += kThreads) {                  // (uniform trip count: the barriers below are reached by all)
        const int k = k0 + tid;
        const int64_t row = (int64_t)b * Kmax + k;
        const bool keep = k < m && kept(det, row, score_thres);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            const long long pos = base + done + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (pos < capacity) {                               // rows beyond the buffer are counted, never stored
                const float* r = det + row * kDetCols;
                const double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], score = r[4], cls = r[5], u = r[6], v = r[7], depth = r[8];
                const double w3 = r[9], h3 = r[10], l3 = r[11], alpha = r[12];
                const double ud = u * depth, vd = v * depth;
                const double x = P[0] * ud + P[1] * vd + P[2] * depth + P[3];
                double y = P[4] * ud + P[5] * vd + P[6] * depth + P[7];
                const double z = P[8] * ud + P[9] * vd + P[10] * depth + P[11];
                y += h3 / 2;
                const double az = atan2(-z, x);
                const double ry = snap_to_pi(alpha + az + kHalfPi, &stuck);
                const double alpha_out = snap_to_pi(ry - az - kHalfPi, &stuck);
                int idx = -1, id = -1;
                if (cls > -2147483648.0 && cls < 2147483648.0) idx = (int)cls - 1;       // .astype(int): towards zero
                else idx = -1;
                if (idx >= 0 && idx < n_lbls) id = class_ids[idx];
                else { idx = -1; bad_class = 1; }
                double* o = rows + pos * 14;
                o[GNMS_KITTI_DET_CLASS] = (double)id;
                o[GNMS_KITTI_DET_ALPHA] = round6(alpha_out, &outside);
                o[GNMS_KITTI_DET_X1 + 0] = round6(x1, &outside);
                o[GNMS_KITTI_DET_X1 + 1] = round6(y1, &outside);
                o[GNMS_KITTI_DET_X1 + 2] = round6(x2, &outside);
                o[GNMS_KITTI_DET_X1 + 3] = round6(y2, &outside);
                o[GNMS_KITTI_DET_H + 0] = round6(h3, &outside);
                o[GNMS_KITTI_DET_H + 1] = round6(w3, &outside);
                o[GNMS_KITTI_DET_H + 2] = round6(l3, &outside);
                o[GNMS_KITTI_DET_T + 0] = round6(x, &outside);
                o[GNMS_KITTI_DET_T + 1] = round6(y, &outside);
                o[GNMS_KITTI_DET_T + 2] = round6(z, &outside);
                o[GNMS_KITTI_DET_RY] = round6(ry, &outside);
                o[GNMS_KITTI_DET_SCORE] = round6(score, &outside);
                if (lbl_index) lbl_index[pos] = idx;
            }
        }
        done += total;
        __syncthreads();                                        // s_wave is rewritten by the next chunk
    }
    if (outside) atomicAdd((unsigned long long*)&state[GNMS_KITTI_ROWS_STATE_OUTSIDE], (unsigned long long)outside);
    const unsigned long long err = (bad_class ? GNMS_KITTI_ROWS_ERR_CLASS : 0) | (stuck ? GNMS_KITTI_ROWS_ERR_ANGLE : 0);
    if (err) atomicOr((unsigned long long*)&state[GNMS_KITTI_ROWS_STATE_ERRORS], err);
    if (tid == 0) {
        const long long end = base + done;
        const long long slot = (long long)image_base + b + 1;
        if (slot < n_offsets) offsets[slot] = end > 2147483647LL ? 2147483647 : (int32_t)end;
        if (b == (int)gridDim.x - 1) state[GNMS_KITTI_ROWS_STATE_PENDING] = end;
    }
}

__global__ void commit_kernel(long long* state, long long images_end) {
    state[GNMS_KITTI_ROWS_STATE_END] = state[GNMS_KITTI_ROWS_STATE_PENDING];
    if (images_end > state[GNMS_KITTI_ROWS_STATE_IMAGES]) state[GNMS_KITTI_ROWS_STATE_IMAGES] = images_end;
}

__global__ __launch_bounds__(kThreads) void round6_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t n, long long* outside_count) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int outside = 0;
    out[i] = round6(in[i], &outside);
    if (outside && outside_count) atomicAdd((unsigned long long*)outside_count, 1ull);
}

}  // namespace

extern "C" int gnms_kitti_rows_append(const float* det, int det_cols, const int32_t* counts, const double* p2_inv, int B, int Kmax,
                                      int nms_topN_post, double score_thres, const int32_t* class_ids, int n_lbls, int32_t* kept_scratch,
                                      double* rows, int32_t* lbl_index, int64_t capacity, int32_t* offsets, int n_offsets, int image_base,
                                      int64_t* state, void* stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "state words are 64-bit");
    GNMS_CHECK_ARG(det_cols == kDetCols, "gnms_kitti_rows_append: det must have %d columns, got %d", kDetCols, det_cols);
    GNMS_CHECK_ARG(B >= 0 && Kmax >= 0, "gnms_kitti_rows_append: negative size (B=%d Kmax=%d)", B, Kmax);
    GNMS_CHECK_ARG(nms_topN_post >= 0, "gnms_kitti_rows_append: negative nms_topN_post (%d)", nms_topN_post);
    GNMS_CHECK_ARG(n_lbls >= 1 && n_lbls <= GNMS_KITTI_ROWS_MAX_LBLS, "gnms_kitti_rows_append: n_lbls (%d) outside 1..%d", n_lbls,
                   GNMS_KITTI_ROWS_MAX_LBLS);
    GNMS_CHECK_ARG(capacity >= 0 && n_offsets >= 1 && image_base >= 0, "gnms_kitti_rows_append: capacity=%lld n_offsets=%d image_base=%d",
                   (long long)capacity, n_offsets, image_base);
    GNMS_CHECK_ARG((int64_t)image_base + B <= 2147483646LL, "gnms_kitti_rows_append: image_base + B overflows");
    GNMS_CHECK_ARG(class_ids && offsets && state && (rows || capacity == 0), "gnms_kitti_rows_append: null pointer");
    GNMS_CHECK_ARG(B == 0 || (counts && p2_inv && kept_scratch && (det || Kmax == 0)), "gnms_kitti_rows_append: null pointer");
    if (B == 0) return GNMS_OK;
    hipStream_t st = (hipStream_t)stream;
    count_kernel<<<B, kThreads, 0, st>>>(det, counts, Kmax, nms_topN_post, score_thres, kept_scratch);
    GNMS_CHECK_LAUNCH();
    write_kernel<<<B, kThreads, 0, st>>>(det, counts, p2_inv, Kmax, nms_topN_post, score_thres, class_ids, n_lbls, kept_scratch, rows, lbl_index,
                                         capacity, offsets, n_offsets, image_base, (long long*)state);
    GNMS_CHECK_LAUNCH();
    commit_kernel<<<1, 1, 0, st>>>((long long*)state, (long long)image_base + B);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_round6(const double* in, double* out, int64_t n, int64_t* outside_count, void* stream) {
    GNMS_CHECK_ARG(n >= 0, "gnms_round6: negative length (%lld)", (long long)n);
    GNMS_CHECK_ARG((in && out) || n == 0, "gnms_round6: null pointer");
    GNMS_CHECK_ARG(n <= (int64_t)2147483647 * kThreads, "gnms_round6: too many elements (%lld)", (long long)n);
    if (n == 0) return GNMS_OK;
    round6_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(in, out, n, (long long*)outside_count);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
