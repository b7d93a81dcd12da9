// heads.hip -- the RPN heads' maps -> the five tensors every entry behind the network reads: what
// models/densenet121_3d_dilate_decomp_alpha.py:166-215 does with a softmax, three sigmoids, fifteen permute-and-copy calls, two
// concatenations and a clone, in one launch, and its backward in one more.
//
//   gnms_heads_assemble            cls / prob / bbox_2d / bbox_3d / acceptance rows [B][R][.] from the maps [B][., H, W]
//   gnms_heads_assemble_backward   the five cotangents (any of them missing = zero) -> the fifteen maps' gradients
//
// Layout: R = A * H * W, anchor row r = (a * H + h) * W + w, so for one map the anchors of an image are consecutive floats and the
// flat anchor n = b * R + r runs over the rows of every output.  A workgroup takes 256 consecutive n: the loads are one lane per
// anchor, fully coalesced per map; the rows narrower or wider than 16 bytes (cls, prob: 4 C bytes, bbox_3d: 40 bytes) are laid down in
// LDS in the order they have in memory, and the tile -- which starts at a multiple of 256 rows, hence 16-byte aligned whatever R and
// the row width are -- is copied out as float4, 64 lanes x 16 contiguous bytes per store instruction.  bbox_2d rows are one float4 per
// lane, acceptance one float per lane: whole lines already.  The backward stages the cotangent rows the same way in the other
// direction and writes planes.  The maps' addresses and batch strides travel in the kernel arguments: no workspace, no atomics,
// nothing filled beforehand, nothing read back, so both entries can be captured into a graph.
#include <limits.h>

#include "gnms_common.h"

namespace {

constexpr int kMaps = 15;                           // cls, x y w h, x3d y3d z3d w3d h3d l3d, alpha, axis, head, acceptance
constexpr int kAcc = 14;
constexpr int kTile = 256;                          // anchors per workgroup = threads per workgroup
constexpr int kCols3d = 10;                         // x3d y3d z3d w3d h3d l3d alpha alpha sigmoid(axis) sigmoid(head)
constexpr int kMinC = 2, kMaxC = 16;

struct HeadMaps { const float* p[kMaps]; long long bs[kMaps]; };
struct GradMaps { float* p[kMaps]; };

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// `count` floats that are contiguous both in LDS and in memory, the memory side 16-byte aligned
__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* lds, int count) {
    const int quads = count >> 2;
    for (int q = threadIdx.x; q < quads; q += kTile) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(lds)[q];
    const int i = (quads << 2) + threadIdx.x;       // (only the last tile of an output can end off a multiple of four)
    if (i < count) dst[i] = lds[i];
}

__device__ __forceinline__ void load_tile(float* lds, const float* __restrict__ src, int count) {
    const int quads = count >> 2;
    for (int q = threadIdx.x; q < quads; q += kTile) reinterpret_cast<float4*>(lds)[q] = reinterpret_cast<const float4*>(src)[q];
    const int i = (quads << 2) + threadIdx.x;
    if (i < count) lds[i] = src[i];
}

// ROW_STORES: every lane writes its own rows straight to memory (the layout the tile copy is measured against, GNMS_HEADS_ROW_STORES=1)
template <bool ROW_STORES>
__global__ __launch_bounds__(kTile) void heads_assemble_kernel(HeadMaps m, long long N, int R, int C, float* __restrict__ cls,
                                                               float* __restrict__ prob, float4* __restrict__ bbox_2d,
                                                               float* __restrict__ bbox_3d, float* __restrict__ acceptance) {
    extern __shared__ float4 heads_lds[];
    float* s_cls = reinterpret_cast<float*>(heads_lds);                 // [kTile][C], then [kTile][C], then [kTile][10]
    float* s_prob = s_cls + kTile * C;
    float* s_b3 = s_prob + kTile * C;
    const int t = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * kTile, n = n0 + t;
    const int rows = (int)(N - n0 < kTile ? N - n0 : kTile);
    if (t < rows) {
        const long long b = n / R;
        const long long r = n - b * R;
        const float* lg = m.p[0] + b * m.bs[0] + r;                     // cls_map[b].flat[c * R + r]
        float* lc = s_cls + t * C;
        float* lp = s_prob + t * C;
        float mx = lg[0];
        lc[0] = mx;
        for (int c = 1; c < C; ++c) {
            const float v = lg[(long long)c * R];
            lc[c] = v;
            mx = fmaxf(mx, v);
        }
        float sum = 0.f;
        for (int c = 0; c < C; ++c) {
            const float e = expf(lc[c] - mx);
            lp[c] = e;
            sum += e;
        }
        for (int c = 0; c < C; ++c) lp[c] = lp[c] / sum;
        float v[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) v[k] = m.p[1 + k][b * m.bs[1 + k] + r];
        bbox_2d[n] = make_float4(v[0], v[1], v[2], v[3]);
        float* l3 = s_b3 + t * kCols3d;
#pragma unroll
        for (int k = 0; k < 6; ++k) l3[k] = v[4 + k];
        l3[6] = v[10];
        l3[7] = v[10];
        l3[8] = sigmoid_f32(v[11]);
        l3[9] = sigmoid_f32(v[12]);
        if (m.p[kAcc]) acceptance[n] = sigmoid_f32(m.p[kAcc][b * m.bs[kAcc] + r]);
        if (ROW_STORES) {
            for (int c = 0; c < C; ++c) {
                cls[n * C + c] = lc[c];
                prob[n * C + c] = lp[c];
            }
#pragma unroll
            for (int k = 0; k < kCols3d; ++k) bbox_3d[n * kCols3d + k] = l3[k];
        }
    }
    if (ROW_STORES) return;
    __syncthreads();
    store_tile(cls + n0 * C, s_cls, rows * C);
    store_tile(prob + n0 * C, s_prob, rows * C);
    store_tile(bbox_3d + n0 * kCols3d, s_b3, rows * kCols3d);
}

// d cls_map[c] = g_cls[c] + p_c (g_prob[c] - sum_j g_prob[j] p_j); d alpha = g3[6] + g3[7]; d axis = g3[8] s (1 - s), head and acceptance
// alike; the other ten maps get their cotangent column.  A cotangent that is NULL is zero; a gradient map that is NULL is not written.
__global__ __launch_bounds__(kTile) void heads_backward_kernel(const float* __restrict__ prob, const float* __restrict__ bbox_3d,
                                                               const float* __restrict__ acceptance, const float* __restrict__ g_cls,
                                                               const float* __restrict__ g_prob, const float4* __restrict__ g_b2,
                                                               const float* __restrict__ g_b3, const float* __restrict__ g_acc,
                                                               long long N, int R, int C, GradMaps g) {
    extern __shared__ float4 heads_lds[];
    float* s_p = reinterpret_cast<float*>(heads_lds);                   // three of [kTile][C], then [kTile][10]
    float* s_gc = s_p + kTile * C;
    float* s_gp = s_gc + kTile * C;
    float* s_g3 = s_gp + kTile * C;
    const int t = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * kTile, n = n0 + t;
    const int rows = (int)(N - n0 < kTile ? N - n0 : kTile);
    const bool want_cls = g.p[0] != nullptr;
    if (want_cls && g_cls) load_tile(s_gc, g_cls + n0 * C, rows * C);
    if (want_cls && g_prob) {
        load_tile(s_gp, g_prob + n0 * C, rows * C);
        load_tile(s_p, prob + n0 * C, rows * C);
    }
    if (g_b3) load_tile(s_g3, g_b3 + n0 * kCols3d, rows * kCols3d);
    __syncthreads();
    if (t >= rows) return;
    const long long b = n / R;
    const long long r = n - b * R;
    if (want_cls) {
        float* d = g.p[0] + b * C * R + r;
        const float* gc = s_gc + t * C;
        const float* gp = s_gp + t * C;
        const float* p = s_p + t * C;
        float dot = 0.f;
        if (g_prob)
            for (int c = 0; c < C; ++c) dot += gp[c] * p[c];
        for (int c = 0; c < C; ++c) {
            float v = g_cls ? gc[c] : 0.f;
            if (g_prob) {
                const float s = p[c] * (gp[c] - dot);
                v = g_cls ? v + s : s;
            }
            d[(long long)c * R] = v;
        }
    }
    const float4 g2 = g_b2 ? g_b2[n] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (g.p[1]) g.p[1][n] = g2.x;
    if (g.p[2]) g.p[2][n] = g2.y;
    if (g.p[3]) g.p[3][n] = g2.z;
    if (g.p[4]) g.p[4][n] = g2.w;
    float g3[kCols3d];
#pragma unroll
    for (int k = 0; k < kCols3d; ++k) g3[k] = g_b3 ? s_g3[t * kCols3d + k] : 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (g.p[5 + k]) g.p[5 + k][n] = g3[k];
    if (g.p[11]) g.p[11][n] = g3[6] + g3[7];
    if (g_b3 && (g.p[12] || g.p[13])) {
        const float2 s = *reinterpret_cast<const float2*>(bbox_3d + n * kCols3d + 8);      // (40 n + 32 bytes: 8-byte aligned)
        g3[8] = g3[8] * s.x * (1.0f - s.x);
        g3[9] = g3[9] * s.y * (1.0f - s.y);
    }
    if (g.p[12]) g.p[12][n] = g3[8];
    if (g.p[13]) g.p[13][n] = g3[9];
    if (g.p[kAcc]) {
        float v = 0.f;
        if (g_acc) {
            const float s = acceptance[n];
            v = g_acc[n] * s * (1.0f - s);
        }
        g.p[kAcc][n] = v;
    }
}

// (developer A/B switch, read once: a process runs one layout; tools/heads_time.py and the test start a child for the other)
bool row_stores() { static const bool on = [] { const char* e = getenv("GNMS_HEADS_ROW_STORES"); return e && e[0] == '1'; }(); return on; }

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

#define GNMS_HEADS_SIZES(what)                                                                                                          \
    GNMS_CHECK_ARG(B >= 0 && A >= 1 && H >= 1 && W >= 1, what ": B=%d (>= 0), A=%d H=%d W=%d (>= 1 each)", B, A, H, W);                 \
    if (C < kMinC || C > kMaxC) {                                                                                                       \
        gnms_set_error(what ": C=%d classes, %d..%d are supported", C, kMinC, kMaxC);                                                   \
        return GNMS_ERR_UNSUPPORTED;                                                                                                    \
    }                                                                                                                                   \
    const long long R = (long long)A * H * W, N = (long long)B * R;                                                                    \
    if (R > INT_MAX || N > (long long)INT_MAX * kTile) {                                                                                \
        gnms_set_error(what ": A*H*W=%lld anchors per image, B*A*H*W=%lld: too many", R, N);                                           \
        return GNMS_ERR_UNSUPPORTED;                                                                                                    \
    }                                                                                                                                   \
    if (N == 0) return GNMS_OK

extern "C" int gnms_heads_assemble(const void* const* maps, const long long* batch_strides, int B, int A, int H, int W, int C, float* cls,
                                   float* prob, float* bbox_2d, float* bbox_3d, float* acceptance, void* stream) {
    GNMS_HEADS_SIZES("gnms_heads_assemble");
    GNMS_CHECK_ARG(maps && batch_strides, "gnms_heads_assemble: maps / batch_strides missing");
    HeadMaps m;
    for (int k = 0; k < kMaps; ++k) {
        GNMS_CHECK_ARG(maps[k] || k == kAcc, "gnms_heads_assemble: map %d is NULL (only the acceptance map, %d, may be)", k, kAcc);
        GNMS_CHECK_ARG(batch_strides[k] >= 0, "gnms_heads_assemble: batch stride %d is negative", k);
        m.p[k] = static_cast<const float*>(maps[k]);
        m.bs[k] = batch_strides[k];
    }
    GNMS_CHECK_ARG(cls && prob && bbox_2d && bbox_3d, "gnms_heads_assemble: null output");
    GNMS_CHECK_ARG(!maps[kAcc] || acceptance, "gnms_heads_assemble: an acceptance map without an acceptance output");
    GNMS_CHECK_ARG(aligned16(cls) && aligned16(prob) && aligned16(bbox_2d) && aligned16(bbox_3d), "gnms_heads_assemble: cls, prob, bbox_2d and bbox_3d must be 16-byte aligned");
    const unsigned grid = (unsigned)((N + kTile - 1) / kTile);
    const size_t lds = sizeof(float) * kTile * (2 * C + kCols3d);
    if (row_stores())
        heads_assemble_kernel<true><<<grid, kTile, lds, (hipStream_t)stream>>>(m, N, (int)R, C, cls, prob, reinterpret_cast<float4*>(bbox_2d), bbox_3d, acceptance);
    else
        heads_assemble_kernel<false><<<grid, kTile, lds, (hipStream_t)stream>>>(m, N, (int)R, C, cls, prob, reinterpret_cast<float4*>(bbox_2d), bbox_3d, acceptance);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_heads_assemble_backward(const float* prob, const float* bbox_3d, const float* acceptance, const float* g_cls,
                                            const float* g_prob, const float* g_bbox_2d, const float* g_bbox_3d, const float* g_acceptance,
                                            int B, int A, int H, int W, int C, void* const* grad_maps, void* stream) {
    GNMS_HEADS_SIZES("gnms_heads_assemble_backward");
    GNMS_CHECK_ARG(grad_maps != nullptr, "gnms_heads_assemble_backward: grad_maps missing");
    GradMaps g;
    for (int k = 0; k < kMaps; ++k) g.p[k] = static_cast<float*>(grad_maps[k]);
    GNMS_CHECK_ARG(!(g_prob && g.p[0]) || prob, "gnms_heads_assemble_backward: the cotangent of prob needs prob");
    GNMS_CHECK_ARG(!(g_bbox_3d && (g.p[12] || g.p[13])) || bbox_3d, "gnms_heads_assemble_backward: the cotangent of bbox_3d needs bbox_3d");
    GNMS_CHECK_ARG(!(g_acceptance && g.p[kAcc]) || acceptance, "gnms_heads_assemble_backward: the cotangent of acceptance needs acceptance");
    GNMS_CHECK_ARG(aligned16(prob) && aligned16(g_cls) && aligned16(g_prob) && aligned16(g_bbox_2d) && aligned16(g_bbox_3d) && (uintptr_t)bbox_3d % 8 == 0,
                   "gnms_heads_assemble_backward: prob and the cotangents of cls, prob, bbox_2d and bbox_3d must be 16-byte aligned, bbox_3d 8-byte");
    const unsigned grid = (unsigned)((N + kTile - 1) / kTile);
    const size_t lds = sizeof(float) * kTile * (3 * C + kCols3d);
    heads_backward_kernel<<<grid, kTile, lds, (hipStream_t)stream>>>(prob, bbox_3d, acceptance, g_cls, g_prob, reinterpret_cast<const float4*>(g_bbox_2d), g_bbox_3d,
                                                                     g_acceptance, N, (int)R, C, g);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
