// sort_bins.h -- the bin function of the histogram sort (sort_hist_rank_body, nms_sort_kernels.h).  Plain C++ without a HIP header, so that a
// host program can include it alone (tests/test_sort_hist_rank.py compiles one and walks sorted keys through it).
//
// The sort's keys order the scores DESCENDING with NaN first, and the x centres ASCENDING with NaN last (gnms_desc_key / column_key).  A bin
// function is usable when it never decreases along that order: then the keys of bin b all stand in front of the keys of bin b + 1, and a
// key's rank is (keys in the bins below its own) + (smaller keys in its own bin).
//
// hist_bin_asc is non-decreasing in the value c, NaN last:
//   - c NaN -> nb - 1 and c = +inf -> nb - 1, the last bin: nothing orders behind them but each other;
//   - c <= lo -> 0: -inf, the finite minimum itself (either zero compares equal to the other), and with lo == hi every finite value;
//   - otherwise f = (c - lo) * scale with scale >= 0.  Subtracting a constant and multiplying by a non-negative constant are monotone under
//     round-to-nearest (and stay so where a result is flushed to zero), f >= 0, the clamp to nb - 1 and the truncation to an integer are
//     monotone.  f is NaN only as inf * 0 (c - lo overflowed while scale = 0: lo == hi or a span that is not finite); then scale is 0 for
//     every key of the image, every other f is 0, and NaN goes to bin 0 with them.
// hist_bin_desc mirrors it: nb - 1 - hist_bin_asc(v) never increases in v, so it never decreases along descending scores, and NaN, the
// first key, gets bin 0.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNMS_BIN_FN __host__ __device__ inline
#else
#define GNMS_BIN_FN inline
#endif

// nb / (hi - lo) for a finite positive span, else 0 (lo, hi: the finite minimum and maximum; +inf, -inf when there is no finite value)
GNMS_BIN_FN float hist_bin_scale(float lo, float hi, unsigned nb) {
    const float span = hi - lo;
    return (span > 0.0f && span < __builtin_inff()) ? (float)nb / span : 0.0f;
}

GNMS_BIN_FN unsigned hist_bin_asc(float c, float lo, float scale, unsigned nb) {
    if (c != c) return nb - 1u;
    if (c == __builtin_inff()) return nb - 1u;
    if (c <= lo) return 0u;
    float f = (c - lo) * scale;
    if (!(f >= 0.0f)) f = 0.0f;
    const float top = (float)(nb - 1u);
    return (unsigned)(f < top ? f : top);
}

GNMS_BIN_FN unsigned hist_bin_desc(float v, float lo, float scale, unsigned nb) {
    if (v != v) return 0u;
    return nb - 1u - hist_bin_asc(v, lo, scale, nb);
}
