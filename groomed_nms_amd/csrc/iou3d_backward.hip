// iou3d_backward.hip -- gnms_iou3d_backward: the cotangent of a pairwise 3D overlap matrix (gnms_iou3d_from_params, method 0 / 1 / 2,
// gnms_nms_overlap3d_from_params) contracted with d overlap / d cuboid.
//
//   d_params_a[b][i] = sum_j grad[b][i][j] * d f(a_i, b_j)/d a_i          d_params_b[b][j] = sum_i grad[b][i][j] * d f(a_i, b_j)/d b_j
//
// Three launches.  iou3d_records_kernel builds the boxes' records (the forward's floats: corners_of + aabb_record; the backward keeps
// the first eight floats of a record).  iou3d_backward_kernel is iou_backward.hip's walker with six accumulators where that has four:
// one WAVE owns a unit of (rc x 32) rows x 128 columns and walks it in chunks of 32 rows x 64 columns; a chunk's cotangents are read
// from memory ONCE into the wave's own 8 KiB of LDS and used twice (column pass: lane = column; row pass: lane = (row, column half)).
// Both sums run in a fixed order, units meet only in memory (slab_a[column tile], slab_b[row tile]).  iou3d_backward_reduce_kernel adds
// the slabs in tile order -- no float atomics, the same bits every run -- and carries the six extent sums of a box to its seven
// parameters (stage 1, once per box).  A chunk, and inside it a wave-step, whose 64 cotangents are all zero skips the arithmetic.
#include "iou3d_grad.h"

namespace {

using namespace gnms_iou3d_grad;

constexpr int kChunkRows = 32;
constexpr int kSubCols = 64;
constexpr int kSubTiles = 2;                     // (the 2D walker has 4: 12 column accumulators here against its 16)
constexpr int kUnitCols = kSubCols * kSubTiles;
constexpr int kUnitsPerWG = 4;                   // waves of a workgroup; they share nothing
constexpr int kRec8 = 8;                         // floats kept per box: u | v of the record

int chunks_per_unit(int B, int M, int N) {
    int rc = 8;
    while (rc > 1 && (long long)B * gnms_div_up(M, kChunkRows * rc) * gnms_div_up(N, kUnitCols) < 8192) rc >>= 1;
    return rc;
}

struct SlabPlan {
    int rc, RT, CT;
    size_t rec_a, rec_b, a_bytes, b_bytes, total;
};
SlabPlan plan_for(int B, int M, int N, bool self) {
    SlabPlan s;
    s.rc = chunks_per_unit(B, M, N);
    s.RT = gnms_div_up(M, kChunkRows * s.rc);
    s.CT = gnms_div_up(N, kUnitCols);
    s.rec_a = gnms_align_up((size_t)B * M * kRec8 * sizeof(float), 256);
    s.rec_b = self ? 0 : gnms_align_up((size_t)B * N * kRec8 * sizeof(float), 256);
    s.a_bytes = gnms_align_up((size_t)B * s.CT * M * 24, 256);
    s.b_bytes = gnms_align_up((size_t)B * s.RT * N * 24, 256);
    s.total = s.rec_a + s.rec_b + s.a_bytes + s.b_bytes;
    return s;
}

__global__ __launch_bounds__(256) void iou3d_records_kernel(const float* __restrict__ params, long count, float* __restrict__ rec) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float4 u, v, e;
    record_of_params(params + i * 7, u, v, e);
    float4* o = reinterpret_cast<float4*>(rec + i * kRec8);
    o[0] = u; o[1] = v;
}

__device__ __forceinline__ float bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ Rec bcast_rec(const Rec& r, int lane) {
    Rec o;
    o.x0 = bcast(r.x0, lane); o.x1 = bcast(r.x1, lane); o.y0 = bcast(r.y0, lane); o.y1 = bcast(r.y1, lane);
    o.z0 = bcast(r.z0, lane); o.z1 = bcast(r.z1, lane); o.vol = bcast(r.vol, lane);
    return o;
}

// orders the wave's own LDS stores and loads (the tile is private to the wave: no workgroup barrier anywhere in this kernel)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int METHOD, bool WANT_A, bool WANT_B>
__global__ __launch_bounds__(256, 3) void iou3d_backward_kernel(const float* __restrict__ RA, const float* __restrict__ RB,
                                                             const float* __restrict__ grad, int M, int N, long ld, int vec, int rc, int RT,
                                                             int CT, long units, float* __restrict__ slab_a, float* __restrict__ slab_b) {
    __shared__ float tiles[kUnitsPerWG][kChunkRows * kSubCols];
    __shared__ float4 crecs[kUnitsPerWG][2 * kSubCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long unit = (long)blockIdx.x * kUnitsPerWG + wave;
    if (unit >= units) return;
    const int ct = (int)(unit % CT), rt = (int)((unit / CT) % RT), img = (int)(unit / ((long)CT * RT));
    const float4* ra4 = reinterpret_cast<const float4*>(RA) + (size_t)img * M * 2;
    const float4* rb4 = reinterpret_cast<const float4*>(RB) + (size_t)img * N * 2;
    const float* g = grad + (size_t)img * M * ld;
    float* t = tiles[wave];
    float4* cb = crecs[wave];
    const int row_begin = rt * rc * kChunkRows;
    const int row_end = min(M, row_begin + rc * kChunkRows);
    const int col0 = ct * kUnitCols;
    const int lrow = lane & 31, half = lane >> 5;

    float accb[kSubTiles][6];
#pragma unroll
    for (int cs = 0; cs < kSubTiles; ++cs)
#pragma unroll
        for (int k = 0; k < 6; ++k) accb[cs][k] = 0.0f;

    for (int r0 = row_begin; r0 < row_end; r0 += kChunkRows) {
        const int myrow = r0 + lrow;                                  // lanes r and r + 32 hold row r0 + r
        const size_t rr2 = (size_t)min(myrow, M - 1) * 2;
        const Rec ra = rec_of(ra4[rr2], ra4[rr2 + 1]);
        float acca[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int cs = 0; cs < kSubTiles; ++cs) {
            const int c0 = col0 + cs * kSubCols;
            if (c0 < N) {
                const int col = c0 + lane;
                const size_t cc2 = (size_t)min(col, N - 1) * 2;
                const float4 cu = rb4[cc2], cv = rb4[cc2 + 1];
                const Rec crec = rec_of(cu, cv);
                // the chunk's cotangents, once: element (r, c) at r * 64 + (c ^ r) -- both passes read the 32 banks conflict-free
                bool nz = false;
                if (vec && c0 + kSubCols <= N) {
                    // 16-byte loads, all eight in flight: a lane takes four columns of rows lane / 16 + 4 i
                    const int rr = lane >> 4, cc = (lane & 15) * 4;
                    const float* gp = g + (size_t)(r0 + rr) * ld + c0 + cc;
                    float4 v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        v[i] = (r0 + rr + 4 * i < row_end) ? *reinterpret_cast<const float4*>(gp + (size_t)(4 * i) * ld) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int r = rr + 4 * i;
                        nz = nz || v[i].x != 0.0f || v[i].y != 0.0f || v[i].z != 0.0f || v[i].w != 0.0f;
                        t[r * kSubCols + (cc ^ r)] = v[i].x;
                        t[r * kSubCols + ((cc + 1) ^ r)] = v[i].y;
                        t[r * kSubCols + ((cc + 2) ^ r)] = v[i].z;
                        t[r * kSubCols + ((cc + 3) ^ r)] = v[i].w;
                    }
                } else {
                    const float* gp = g + (size_t)r0 * ld + min(col, N - 1);
#pragma unroll 8
                    for (int r = 0; r < kChunkRows; ++r) {
                        const float v = (r0 + r < row_end && col < N) ? gp[(size_t)r * ld] : 0.0f;
                        nz = nz || v != 0.0f;
                        t[r * kSubCols + (lane ^ r)] = v;
                    }
                }
                if (__ballot(nz) != 0ull) {
                    if (WANT_A) { cb[2 * lane] = cu; cb[2 * lane + 1] = cv; }
                    wave_lds_fence();
                    if (WANT_B) {
                        for (int r = 0; r < kChunkRows; ++r) {
                            const float v = t[r * kSubCols + (lane ^ r)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const Rec rb = bcast_rec(ra, r);
                            const Pair p = pair_of(rb, crec);
                            add_extent_grad<METHOD>(crec, rb, p, v, accb[cs]);
                        }
                    }
                    if (WANT_A) {
                        for (int j = 0; j < 32; ++j) {
                            const int c = 32 * half + j;
                            const float v = t[lrow * kSubCols + (c ^ lrow)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const Rec ob = rec_of(cb[2 * c], cb[2 * c + 1]);
                            const Pair p = pair_of(ra, ob);
                            add_extent_grad<METHOD>(ra, ob, p, v, acca);
                        }
                    }
                    wave_lds_fence();                                 // the next chunk's stores come after these loads
                }
            }
        }
        if (WANT_A) {
#pragma unroll
            for (int k = 0; k < 6; ++k) acca[k] = acca[k] + __shfl_down(acca[k], 32);     // columns 0..31 + columns 32..63
            if (half == 0 && myrow < row_end) {
                float2* o = reinterpret_cast<float2*>(slab_a + (((size_t)img * CT + ct) * M + myrow) * 6);
                o[0] = make_float2(acca[0], acca[1]); o[1] = make_float2(acca[2], acca[3]); o[2] = make_float2(acca[4], acca[5]);
            }
        }
    }
    if (WANT_B) {
#pragma unroll
        for (int cs = 0; cs < kSubTiles; ++cs) {
            const int col = col0 + cs * kSubCols + lane;
            if (col < N) {
                float2* o = reinterpret_cast<float2*>(slab_b + (((size_t)img * RT + rt) * N + col) * 6);
                o[0] = make_float2(accb[cs][0], accb[cs][1]); o[1] = make_float2(accb[cs][2], accb[cs][3]); o[2] = make_float2(accb[cs][4], accb[cs][5]);
            }
        }
    }
}

__device__ __forceinline__ void add6(float (&s)[6], const float* __restrict__ v) {
    const float2 a = reinterpret_cast<const float2*>(v)[0], b = reinterpret_cast<const float2*>(v)[1], c = reinterpret_cast<const float2*>(v)[2];
    s[0] += a.x; s[1] += a.y; s[2] += b.x; s[3] += b.y; s[4] += c.x; s[5] += c.y;
}

// blockIdx.z = 0: the extent sums of a_i = slab_a[0][i] + slab_a[1][i] + ... (then, self: + slab_b[0][i] + ...); 1: those of b_j from
// slab_b.  Then stage 1 on the box's own parameters and seven stores.
__global__ __launch_bounds__(256) void iou3d_backward_reduce_kernel(const float* __restrict__ slab_a, const float* __restrict__ slab_b,
                                                                    const float* __restrict__ params_a, const float* __restrict__ params_b, int M,
                                                                    int N, int CT, int RT, float* __restrict__ d_a, float* __restrict__ d_b, int self) {
    const int img = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float G[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[7];
    if (blockIdx.z == 0) {
        if (!d_a || i >= M) return;
        for (int ct = 0; ct < CT; ++ct) add6(G, slab_a + (((size_t)img * CT + ct) * M + i) * 6);
        if (self)
            for (int rt = 0; rt < RT; ++rt) add6(G, slab_b + (((size_t)img * RT + rt) * N + i) * 6);
        const size_t o = ((size_t)img * M + i) * 7;
        params_grad(params_a + o, G, d);
#pragma unroll
        for (int k = 0; k < 7; ++k) d_a[o + k] = d[k];
    } else {
        if (!d_b || i >= N) return;
        for (int rt = 0; rt < RT; ++rt) add6(G, slab_b + (((size_t)img * RT + rt) * N + i) * 6);
        const size_t o = ((size_t)img * N + i) * 7;
        params_grad(params_b + o, G, d);
#pragma unroll
        for (int k = 0; k < 7; ++k) d_b[o + k] = d[k];
    }
}

template <int METHOD>
void launch_walker(bool want_a, bool want_b, dim3 grid, hipStream_t st, const float* ra, const float* rb, const float* grad, int M, int N, long ld,
                   int vec, const SlabPlan& s, long units, float* slab_a, float* slab_b) {
#define GNMS_IOU3D_BWD(WA, WB) \
    iou3d_backward_kernel<METHOD, WA, WB><<<grid, 64 * kUnitsPerWG, 0, st>>>(ra, rb, grad, M, N, ld, vec, s.rc, s.RT, s.CT, units, slab_a, slab_b)
    if (want_a && want_b) GNMS_IOU3D_BWD(true, true);
    else if (want_a) GNMS_IOU3D_BWD(true, false);
    else GNMS_IOU3D_BWD(false, true);
#undef GNMS_IOU3D_BWD
}

}  // namespace

extern "C" size_t gnms_iou3d_backward_workspace_bytes(int B, int M, int N) {
    if (B <= 0 || M <= 0 || N <= 0) return 0;
    return plan_for(B, M, N, false).total;                            // (the one-set form needs no second record array: it fits as well)
}

extern "C" int gnms_iou3d_backward(const float* params_a, const float* params_b, const float* grad, int B, int M, int N, int64_t ld, int method,
                                   float* d_params_a, float* d_params_b, void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && M >= 0 && N >= 0, "gnms_iou3d_backward: negative size (B=%d M=%d N=%d)", B, M, N);
    GNMS_CHECK_ARG(method >= 0 && method <= 2, "gnms_iou3d_backward: method %d not in {0,1,2}", method);
    GNMS_CHECK_ARG(d_params_a || d_params_b, "gnms_iou3d_backward: both outputs are NULL");
    const bool self = params_b == nullptr;
    if (self) {
        GNMS_CHECK_ARG(M == N, "gnms_iou3d_backward: params_b is NULL (params_a on both sides) but M (%d) != N (%d)", M, N);
        GNMS_CHECK_ARG(d_params_a && !d_params_b, "gnms_iou3d_backward: params_b is NULL: both roles are summed into d_params_a, d_params_b must be NULL");
    }
    GNMS_CHECK_ARG(ld >= N, "gnms_iou3d_backward: ld (%lld) < N (%d)", (long long)ld, N);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return GNMS_OK;
    if (M == 0 || N == 0) {                                           // no pair: every element that exists is written, with 0
        if (d_params_a && M > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_params_a, 0, sizeof(float) * 7 * (size_t)B * M, st));
        if (d_params_b && N > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_params_b, 0, sizeof(float) * 7 * (size_t)B * N, st));
        return GNMS_OK;
    }
    GNMS_CHECK_ARG(params_a && grad, "gnms_iou3d_backward: null params_a / grad");
    GNMS_CHECK_ARG(workspace != nullptr, "gnms_iou3d_backward: workspace is NULL");
    GNMS_CHECK_ARG((uintptr_t)workspace % 256 == 0, "gnms_iou3d_backward: workspace must be 256-byte aligned");
    const SlabPlan s = plan_for(B, M, N, self);
    if (workspace_bytes < (self ? s.total : gnms_iou3d_backward_workspace_bytes(B, M, N))) {
        gnms_set_error("gnms_iou3d_backward: workspace too small (%zu < %zu)", workspace_bytes, gnms_iou3d_backward_workspace_bytes(B, M, N));
        return GNMS_ERR_WORKSPACE;
    }
    char* w = static_cast<char*>(workspace);
    float* rec_a = reinterpret_cast<float*>(w);
    float* rec_b = self ? rec_a : reinterpret_cast<float*>(w + s.rec_a);
    float* slab_a = reinterpret_cast<float*>(w + s.rec_a + s.rec_b);
    float* slab_b = reinterpret_cast<float*>(w + s.rec_a + s.rec_b + s.a_bytes);
    const long na = (long)B * M, nb = (long)B * N;
    iou3d_records_kernel<<<(unsigned)((na + 255) / 256), 256, 0, st>>>(params_a, na, rec_a);
    GNMS_CHECK_LAUNCH();
    if (!self) {
        iou3d_records_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, st>>>(params_b, nb, rec_b);
        GNMS_CHECK_LAUNCH();
    }
    const bool want_a = d_params_a != nullptr, want_b = self || d_params_b != nullptr;
    const long units = (long)B * s.RT * s.CT;
    const dim3 grid((unsigned)((units + kUnitsPerWG - 1) / kUnitsPerWG));
    const int vec = (ld % 4 == 0) && ((uintptr_t)grad % 16 == 0);   // 16-byte loads of the cotangent
    if (method == 0) launch_walker<0>(want_a, want_b, grid, st, rec_a, rec_b, grad, M, N, (long)ld, vec, s, units, slab_a, slab_b);
    else if (method == 1) launch_walker<1>(want_a, want_b, grid, st, rec_a, rec_b, grad, M, N, (long)ld, vec, s, units, slab_a, slab_b);
    else launch_walker<2>(want_a, want_b, grid, st, rec_a, rec_b, grad, M, N, (long)ld, vec, s, units, slab_a, slab_b);
    GNMS_CHECK_LAUNCH();
    iou3d_backward_reduce_kernel<<<dim3(gnms_div_up(M > N ? M : N, 256), B, self ? 1 : 2), 256, 0, st>>>(
        slab_a, slab_b, params_a, self ? params_a : params_b, M, N, s.CT, s.RT, d_params_a, d_params_b, self ? 1 : 0);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
