// preprocess.hip -- the image front end of lib/augmentations.py (Augmentation / Preprocess) for a whole batch in one
// launch: mirror, bilinear resample to the target height, crop or pad to the target width, normalise, BGR -> RGB planes.
//
//   gnms_preprocess_images   uint8 HWC BGR images of any sizes in one buffer + a descriptor table -> float32 [B][3][H_out][W_out]
//
// Per output pixel, in the reference's order: RandomMirror (the source column is W - 1 - x), Resize (two source rows, two source columns:
// the horizontal pass, then the vertical pass, each one product per tap and one sum, float32), the crop / the zero padding on the right
// edge, Normalize (x / 255, - mean[c], / std[c]; three float32 operations, the padding included, entry 0 on the BLUE channel) and the
// channel swap of lib/imdb_util.py:522-526 / Preprocess.__call__.  -ffp-contract=off (build.py) keeps every operation its own rounding,
// so at a scale of 1 (weights 1 and 0) the result is NumPy's bit for bit.
//
// No workspace, no atomics; buffer and table are read on the device, so a captured launch reads them again at every replay.
#include <limits.h>

#include "gnms_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuad = 4;                                // output pixels of one row per thread: one 16-byte store per plane
constexpr long long kMaxSide = 1ll << 20;               // H, W of a source image

struct norm_consts {
    float mean[3], stdv[3];                             // in the order the reference applies them: entry 0 -> blue
};

// (d + 0.5) * scale - 0.5 in double, rounded to float; floor and fraction; both taps clamped to [0, n - 1]
__device__ __forceinline__ void source_taps(int d, double scale, int n, int& i0, int& i1, float& f) {
    const float s = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(s);
    f = s - fl;
    const int i = (int)fl;
    i0 = min(max(i, 0), n - 1);
    i1 = min(max(i + 1, 0), n - 1);
}

// One thread: four neighbouring pixels of one output row, all three channels.  The 2 x 2 x 3 source bytes per pixel are plain byte
// loads (a few hundred bytes per wave, from two source rows: cached); the stores are one float4 per plane when the output rows are
// 16-byte aligned (kVector: W_out % 4 == 0; a kernel of its own, or the compiler splits the store to share code with the other path),
// per element otherwise.
template <bool kVector>
__global__ __launch_bounds__(kThreads) void preprocess_kernel(const uint8_t* __restrict__ src, long long src_bytes,
                                                              const long long* __restrict__ table, int H_out, int W_out, int quads,
                                                              norm_consts nm, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long* __restrict__ d = table + (size_t)b * GNMS_PREPROCESS_DESC;
    const long long off = d[0], H = d[1], W = d[2], w_rs = d[3];
    const bool mirror = d[4] != 0;
    // uniform per image: a descriptor that does not lie inside the buffer reads nothing and writes nothing
    if (off < 0 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || w_rs < 0 || w_rs > INT_MAX) return;
    if (H * W * 3 > src_bytes || off > src_bytes - H * W * 3) return;
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long long)H_out * quads) return;
    const int y = (int)(idx / quads), x_first = (int)(idx - (long long)y * quads) * kQuad;

    const uint8_t* __restrict__ im = src + off;
    const int h = (int)H, w = (int)W;
    int y0, y1;
    float fy;
    source_taps(y, (double)h / (double)H_out, h, y0, y1, fy);
    const float wy0 = 1.f - fy;
    const uint8_t* __restrict__ row0 = im + (size_t)y0 * w * 3;
    const uint8_t* __restrict__ row1 = im + (size_t)y1 * w * 3;
    const double scale_x = w_rs > 0 ? (double)w / (double)w_rs : 1.0;

    float v[3][kQuad];
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const int x = x_first + k;
        if (x < (int)w_rs) {                                                      // also x < W_out wherever it is stored
            int x0, x1;
            float fx;
            source_taps(x, scale_x, w, x0, x1, fx);
            if (mirror) { x0 = w - 1 - x0; x1 = w - 1 - x1; }
            const float wx0 = 1.f - fx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = (float)row0[x0 * 3 + c] * wx0 + (float)row0[x1 * 3 + c] * fx;     // horizontal pass, upper row
                const float e = (float)row1[x0 * 3 + c] * wx0 + (float)row1[x1 * 3 + c] * fx;     // lower row
                v[c][k] = a * wy0 + e * fy;                                                       // vertical pass
            }
        } else {
            v[0][k] = v[1][k] = v[2][k] = 0.f;                                    // np.pad(..., 'constant'), before Normalize
        }
    }
    const size_t plane = (size_t)H_out * W_out;
    float* __restrict__ o = out + (size_t)b * 3 * plane + (size_t)y * W_out + x_first;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float r[kQuad];
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            float t = v[c][k] / 255.0f;
            t = t - nm.mean[c];
            r[k] = t / nm.stdv[c];
        }
        float* __restrict__ p = o + (size_t)(2 - c) * plane;                      // BGR -> RGB planes
        if (kVector) {
            *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kQuad; ++k)
                if (x_first + k < W_out) p[k] = r[k];
        }
    }
}

}  // namespace

extern "C" int gnms_preprocess_images(const uint8_t* src, int64_t src_bytes, const int64_t* table, int B, int H_out, int W_out,
                                      const float* means, const float* stds, float* out, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && H_out >= 1 && W_out >= 1, "gnms_preprocess_images: B=%d H_out=%d W_out=%d (B >= 0, sizes >= 1)", B, H_out, W_out);
    GNMS_CHECK_ARG(B <= 65535, "gnms_preprocess_images: B=%d images in one launch, 65535 are supported", B);
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(src && table && out && means && stds, "gnms_preprocess_images: src / table / means / stds / out missing");
    GNMS_CHECK_ARG(src_bytes >= 0, "gnms_preprocess_images: src_bytes=%lld", (long long)src_bytes);
    GNMS_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 7) == 0, "gnms_preprocess_images: out must be 16-byte, table 8-byte aligned");
    const int quads = gnms_div_up(W_out, kQuad);
    const long long threads = (long long)H_out * quads;
    GNMS_CHECK_ARG(threads <= (long long)INT_MAX, "gnms_preprocess_images: H_out=%d W_out=%d: too large", H_out, W_out);
    norm_consts nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = means[c];
        nm.stdv[c] = stds[c];
    }
    const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads), (unsigned)B);
    if ((W_out & (kQuad - 1)) == 0)
        preprocess_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(src, (long long)src_bytes, (const long long*)table, H_out, W_out, quads, nm, out);
    else
        preprocess_kernel<false><<<grid, kThreads, 0, (hipStream_t)stream>>>(src, (long long)src_bytes, (const long long*)table, H_out, W_out, quads, nm, out);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
