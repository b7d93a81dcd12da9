// bbox_stats.hip -- the reduction over the data set of compute_bbox_stats (lib/rpn_util.py:547-736): from the raw
// transforms of gnms_compute_targets to bbox_means / bbox_stds.
//
//   gnms_bbox_stats_partials   per image of a batch: the foreground rows (transforms[:, 4] > 0) in anchor order, their count, and per
//                              statistics column either the float32 sum NumPy's np.sum(..., axis=0) gives (:642-643) or, given the
//                              means, the float64 sum of squared deviations (:712-713); written at the image's position in the data set
//   gnms_bbox_stats_finish     the partials of the whole data set in image order, in double-double -> the 13 means (:652) or the
//                              13 deviations (:721), rounded to float64 once
//
// No atomics, no workspace, nothing filled beforehand, nothing read back; every addition happens in an order the inputs alone fix, so
// the result depends neither on the batch size, nor on the order the batches come in, nor on the run.
#include <limits.h>

#include "gnms_common.h"

namespace {

constexpr int kCols = GNMS_BBOX_STATS_COLS;          // transforms[:, 0:4] and transforms[:, 5:14]
constexpr int kThreads = 512;                        // gnms_bbox_stats_partials: one workgroup per image
constexpr int kWaves = kThreads / GNMS_WAVE;
constexpr int kUnroll = 4;                           // label loads in flight per lane
constexpr int kMasks = kWaves * kUnroll;             // 64-row ballots per step of kMasks * 64 = 2048 rows
static_assert(kMasks <= GNMS_WAVE, "one lane of wave 0 per ballot");

// One workgroup per image.  All waves read the label column, 2048 rows a step, and leave one ballot per 64 rows in LDS (two sets, so
// one barrier a step is enough: a set is written again only after the barrier that follows its reading).  Wave 0 then walks the set
// bits in ascending order -- the foreground rows in anchor order, the compaction of np.flatnonzero without the list -- with lane c
// adding column c: a plain sequential sum, which is the order NumPy's axis-0 reduction of a C-contiguous [m, k] array uses.
template <bool kDeviation>
__global__ __launch_bounds__(kThreads) void image_partials_kernel(const float* __restrict__ transforms, int R, long long ld,
                                                                  const int32_t* __restrict__ image_ids, int n_images,
                                                                  const double* __restrict__ means, float* __restrict__ sums,
                                                                  double* __restrict__ sq_sums, int32_t* __restrict__ counts) {
    __shared__ unsigned long long s_mask[2][kMasks];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (GNMS_WAVE - 1), wave = t / GNMS_WAVE;
    const int img = image_ids[b];
    if (img < 0 || img >= n_images) return;                                          // uniform: nothing is written out of bounds
    const float* __restrict__ tr = transforms + (size_t)b * (size_t)R * (size_t)ld;
    const int c = lane < kCols ? lane : 0;
    const int col = c < 4 ? c : c + 1;
    const double mean = kDeviation ? means[c] : 0.0;
    float s32 = 0.f;
    double s64 = 0.0;
    int n = 0;
    constexpr int kStep = kMasks * GNMS_WAVE;
    for (int base = 0, step = 0; base < R; base += kStep, ++step) {
        float lbl[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const long long r = (long long)base + (wave * kUnroll + k) * GNMS_WAVE + lane;
            lbl[k] = r < R ? tr[(size_t)r * ld + 4] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned long long m = __ballot(lbl[k] > 0.f);                     // :629
            if (lane == 0) s_mask[step & 1][wave * kUnroll + k] = m;
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned long long mine = lane < kMasks ? s_mask[step & 1][lane] : 0ull;
            unsigned long long any = __ballot(mine != 0ull);
            while (any) {
                const int w = __ffsll((long long)any) - 1;
                any &= any - 1ull;
                unsigned long long m = s_mask[step & 1][w];
                const long long first = (long long)base + (long long)w * GNMS_WAVE;
                if (lane < kCols) {
                    while (m) {
                        const int j = __ffsll((long long)m) - 1;
                        m &= m - 1ull;
                        const float x = tr[(size_t)(first + j) * ld + col];
                        if (kDeviation) {
                            const double d = (double)x - mean;
                            s64 += d * d;
                        } else {
                            s32 += x;                                                // from +0, as np.sum's axis-0 reduction does
                        }
                        ++n;
                    }
                } else {
                    n += __popcll(m);
                }
            }
        }
    }
    if (wave == 0) {
        if (lane < kCols) {
            if (kDeviation) sq_sums[(size_t)img * kCols + lane] = s64;
            else sums[(size_t)img * kCols + lane] = s32;
        }
        if (lane == kCols) counts[img] = n;
    }
}

struct dd { double hi, lo; };

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd a, double x) {
    const dd s = two_sum(a.hi, x);
    const double lo = s.lo + a.lo, hi = s.hi + lo;
    return {hi, lo - (hi - s.hi)};
}
// a / b; the quotient's two leading terms, normalised
__device__ __forceinline__ dd dd_div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    const double p = q1 * b.hi, pe = fma(q1, b.hi, -p) + q1 * b.lo;                  // q1 * b
    const double r = ((a.hi - p) - pe) + a.lo;
    const double q2 = r / b.hi;
    const double hi = q1 + q2;
    return {hi, q2 - (hi - q1)};
}

// One wave.  Lane c adds the partials of column c over the images in order; every lane adds the counts (int64).
__global__ __launch_bounds__(GNMS_WAVE) void finish_kernel(int deviation, const uint8_t* __restrict__ used, int n_images,
                                                           const float* __restrict__ sums, const double* __restrict__ sq_sums,
                                                           const int32_t* __restrict__ counts, long long* __restrict__ count,
                                                           double* __restrict__ out) {
    const int lane = threadIdx.x, c = lane < kCols ? lane : 0;
    dd acc = {0.0, 0.0};
    long long n = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!used[i]) continue;                                                      // :587: an image without ground truths
        const int m = counts[i];
        if (m <= 0) continue;                                                        // :631
        n += m;
        acc = dd_add(acc, deviation ? sq_sums[(size_t)i * kCols + c] : (double)sums[(size_t)i * kCols + c]);
    }
    if (deviation) n = count[0];                                                     // :721 divides by the mean pass's count
    else if (lane == 0) count[0] = n;
    const dd den = two_sum((double)n, 1e-10);                                        // :579
    const dd q = dd_div(acc, den);
    double v = q.hi;
    if (deviation) {
        const double x = sqrt(q.hi);
        v = x > 0.0 ? x + (fma(-x, x, q.hi) + q.lo) / (2.0 * x) : x;
    }
    if (lane < kCols) out[lane] = v;
}

}  // namespace

extern "C" int gnms_bbox_stats_partials(const float* transforms, int B, int R, int64_t ld, const int32_t* image_ids, int n_images,
                                        const double* means, float* sums, double* sq_sums, int32_t* counts, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && R >= 0 && n_images >= 0, "gnms_bbox_stats_partials: B=%d R=%d n_images=%d (>= 0 each)", B, R, n_images);
    GNMS_CHECK_ARG(ld >= 14, "gnms_bbox_stats_partials: ld=%lld, the transforms of decomp_alpha have >= 14 columns", (long long)ld);
    GNMS_CHECK_ARG(R <= INT_MAX - kMasks * GNMS_WAVE, "gnms_bbox_stats_partials: R=%d: too many", R);
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(B <= n_images, "gnms_bbox_stats_partials: B=%d images in the batch, n_images=%d in the data set", B, n_images);
    GNMS_CHECK_ARG(image_ids && counts, "gnms_bbox_stats_partials: image_ids / counts missing");
    GNMS_CHECK_ARG(R == 0 || transforms, "gnms_bbox_stats_partials: transforms missing");
    GNMS_CHECK_ARG(means ? (sq_sums != nullptr) : (sums != nullptr),
                   "gnms_bbox_stats_partials: the mean pass (means NULL) writes sums, the deviation pass sq_sums");
    if (means)
        image_partials_kernel<true><<<(unsigned)B, kThreads, 0, (hipStream_t)stream>>>(transforms, R, (long long)ld, image_ids, n_images, means,
                                                                                       sums, sq_sums, counts);
    else
        image_partials_kernel<false><<<(unsigned)B, kThreads, 0, (hipStream_t)stream>>>(transforms, R, (long long)ld, image_ids, n_images, means,
                                                                                        sums, sq_sums, counts);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_bbox_stats_finish(int deviation, const uint8_t* used, int n_images, const float* sums, const double* sq_sums,
                                      const int32_t* counts, long long* count, double* out, void* stream) {
    GNMS_CHECK_ARG(n_images >= 0, "gnms_bbox_stats_finish: n_images=%d (>= 0)", n_images);
    GNMS_CHECK_ARG(count && out, "gnms_bbox_stats_finish: count / out missing");
    GNMS_CHECK_ARG(n_images == 0 || (used && counts), "gnms_bbox_stats_finish: used / counts missing");
    GNMS_CHECK_ARG(n_images == 0 || (deviation ? (sq_sums != nullptr) : (sums != nullptr)),
                   "gnms_bbox_stats_finish: the mean pass reads sums, the deviation pass sq_sums");
    finish_kernel<<<1, GNMS_WAVE, 0, (hipStream_t)stream>>>(deviation ? 1 : 0, used, n_images, sums, sq_sums, counts, count, out);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
