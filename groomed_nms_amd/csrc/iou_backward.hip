// iou_backward.hip -- gnms_iou2d_backward: the cotangent of a pairwise 2D IoU matrix contracted with dIoU/dbox.
//
//   d_boxes_a[b][i] = sum_j grad[b][i][j] * dIoU(a_i, b_j)/da_i          d_boxes_b[b][j] = sum_i grad[b][i][j] * dIoU(a_i, b_j)/db_j
//
// One WAVE owns a unit of (rc x 32) rows x 256 columns and walks it in chunks of 32 rows x 64 columns.  A chunk's cotangents are read
// from memory ONCE (16-byte loads where ld and the pointer allow, else lane = column) into the wave's own 8 KiB of LDS, and used twice:
//   column pass: lane = column, the 32 rows one after the other   -> four accumulators per column, kept in registers down the unit
//   row pass   : lane = (row, column half), 32 columns each       -> four accumulators per row, the halves added (low + high)
// Both sums run in a fixed order.  Units meet only in memory: a unit stores its row sums into slab_a[column tile] and its column sums
// into slab_b[row tile], and iou2d_backward_reduce_kernel adds the slabs in tile order -- no float atomics, the same bits every run.
// A chunk, and inside it a wave-step, whose 64 cotangents are all zero skips the arithmetic: the masked-group layer's matrix gradient
// has one non-zero per row, and this kernel then runs at the speed of the read.
#include "iou_grad.h"

namespace {

using namespace gnms_iou_grad;

constexpr int kChunkRows = 32;
constexpr int kSubCols = 64;
constexpr int kSubTiles = 4;
constexpr int kUnitCols = kSubCols * kSubTiles;
constexpr int kUnitsPerWG = 4;                   // waves of a workgroup; they share nothing

// 32-row chunks per unit: 8 (256 rows) unless that leaves the chip short of waves.  A wave loads a chunk, then works on it, so the read
// is hidden by OTHER waves: 12 resident per CU (__launch_bounds__(256, 3): 156 VGPRs, no spill; 4 per SIMD spills 38) and a few rounds
// of them -- 8192 units -- before the units grow.  B = 8, N = 4096: 2 chunks per unit, 33 MB of column slabs beside the 512 MB matrix.
int chunks_per_unit(int B, int M, int N) {
    int rc = 8;
    while (rc > 1 && (long long)B * gnms_div_up(M, kChunkRows * rc) * gnms_div_up(N, kUnitCols) < 8192) rc >>= 1;
    return rc;
}

struct SlabPlan {
    int rc, RT, CT;
    size_t a_bytes, b_bytes;
};
SlabPlan plan_for(int B, int M, int N) {
    SlabPlan s;
    s.rc = chunks_per_unit(B, M, N);
    s.RT = gnms_div_up(M, kChunkRows * s.rc);
    s.CT = gnms_div_up(N, kUnitCols);
    s.a_bytes = gnms_align_up((size_t)B * s.CT * M * 16, 256);
    s.b_bytes = gnms_align_up((size_t)B * s.RT * N * 16, 256);
    return s;
}

__device__ __forceinline__ float4 bcast4(const float4 v, int lane) {
    return make_float4(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), lane)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), lane)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.z), lane)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.w), lane)));
}

// orders the wave's own LDS stores and loads (the tile is private to the wave: no workgroup barrier anywhere in this kernel)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <bool WANT_A, bool WANT_B>
__global__ __launch_bounds__(256, 3) void iou2d_backward_kernel(const float* __restrict__ A, const float* __restrict__ Bx,
                                                             const float* __restrict__ grad, int M, int N, long ld, int vec, int rc, int RT,
                                                             int CT, long units, float* __restrict__ slab_a, float* __restrict__ slab_b) {
    __shared__ float tiles[kUnitsPerWG][kChunkRows * kSubCols];
    __shared__ float4 cboxes[kUnitsPerWG][kSubCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long unit = (long)blockIdx.x * kUnitsPerWG + wave;
    if (unit >= units) return;
    const int ct = (int)(unit % CT), rt = (int)((unit / CT) % RT), img = (int)(unit / ((long)CT * RT));
    const float* a = A + (size_t)img * M * 4;
    const float* bx = Bx + (size_t)img * N * 4;
    const float* g = grad + (size_t)img * M * ld;
    float* t = tiles[wave];
    float4* cb = cboxes[wave];
    const int row_begin = rt * rc * kChunkRows;
    const int row_end = min(M, row_begin + rc * kChunkRows);
    const int col0 = ct * kUnitCols;
    const int lrow = lane & 31, half = lane >> 5;

    float accb[kSubTiles][4];
#pragma unroll
    for (int cs = 0; cs < kSubTiles; ++cs) accb[cs][0] = accb[cs][1] = accb[cs][2] = accb[cs][3] = 0.0f;

    for (int r0 = row_begin; r0 < row_end; r0 += kChunkRows) {
        const int myrow = r0 + lrow;                                  // lanes r and r + 32 hold row r0 + r
        const float4 ra = *reinterpret_cast<const float4*>(a + (size_t)min(myrow, M - 1) * 4);
        const float rarea = box_area(ra);
        float acca[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int cs = 0; cs < kSubTiles; ++cs) {
            const int c0 = col0 + cs * kSubCols;
            if (c0 < N) {
                const int col = c0 + lane;
                const float4 cbox = *reinterpret_cast<const float4*>(bx + (size_t)min(col, N - 1) * 4);
                const float carea = box_area(cbox);
                // the chunk's cotangents, once: element (r, c) at r * 64 + (c ^ r) -- both passes read the 32 banks conflict-free
                bool nz = false;
                if (vec && c0 + kSubCols <= N) {
                    // 16-byte loads, all eight in flight: a lane takes four columns of rows lane / 16 + 4 i (8 KiB per wave on its way)
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
                    const float* gp = g + (size_t)r0 * ld + col;
#pragma unroll 8
                    for (int r = 0; r < kChunkRows; ++r) {
                        const float v = (r0 + r < row_end && col < N) ? gp[(size_t)r * ld] : 0.0f;
                        nz = nz || v != 0.0f;
                        t[r * kSubCols + (lane ^ r)] = v;
                    }
                }
                if (__ballot(nz) != 0ull) {
                    if (WANT_A) cb[lane] = cbox;
                    wave_lds_fence();
                    if (WANT_B) {
                        for (int r = 0; r < kChunkRows; ++r) {
                            const float v = t[r * kSubCols + (lane ^ r)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const float4 rb = bcast4(ra, r);
                            const float rbarea = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rarea), r));
                            const Pair p = pair_of(rb, rbarea, cbox, carea);
                            add_box_grad(cbox, rb, p, v, accb[cs]);
                        }
                    }
                    if (WANT_A) {
                        for (int j = 0; j < 32; ++j) {
                            const int c = 32 * half + j;
                            const float v = t[lrow * kSubCols + (c ^ lrow)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const float4 ob = cb[c];
                            const Pair p = pair_of(ra, rarea, ob, box_area(ob));
                            add_box_grad(ra, ob, p, v, acca);
                        }
                    }
                    wave_lds_fence();                                 // the next chunk's stores come after these loads
                }
            }
        }
        if (WANT_A) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acca[k] = acca[k] + __shfl_down(acca[k], 32);     // columns 0..31 + columns 32..63
            if (half == 0 && myrow < row_end)
                *reinterpret_cast<float4*>(slab_a + (((size_t)img * CT + ct) * M + myrow) * 4) = make_float4(acca[0], acca[1], acca[2], acca[3]);
        }
    }
    if (WANT_B) {
#pragma unroll
        for (int cs = 0; cs < kSubTiles; ++cs) {
            const int col = col0 + cs * kSubCols + lane;
            if (col < N)
                *reinterpret_cast<float4*>(slab_b + (((size_t)img * RT + rt) * N + col) * 4) =
                    make_float4(accb[cs][0], accb[cs][1], accb[cs][2], accb[cs][3]);
        }
    }
}

__device__ __forceinline__ void add4(float4& s, const float4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }

// blockIdx.z = 0: d_boxes_a[i] = slab_a[0][i] + slab_a[1][i] + ... (then, self: + slab_b[0][i] + ...); 1: d_boxes_b from slab_b
__global__ __launch_bounds__(256) void iou2d_backward_reduce_kernel(const float* __restrict__ slab_a, const float* __restrict__ slab_b, int M, int N,
                                                                    int CT, int RT, float* __restrict__ d_a, float* __restrict__ d_b, int self) {
    const int img = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float4* sa = reinterpret_cast<const float4*>(slab_a);
    const float4* sb = reinterpret_cast<const float4*>(slab_b);
    if (blockIdx.z == 0) {
        if (!d_a || i >= M) return;
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int ct = 0; ct < CT; ++ct) add4(s, sa[((size_t)img * CT + ct) * M + i]);
        if (self)
            for (int rt = 0; rt < RT; ++rt) add4(s, sb[((size_t)img * RT + rt) * N + i]);
        reinterpret_cast<float4*>(d_a)[(size_t)img * M + i] = s;
    } else {
        if (!d_b || i >= N) return;
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int rt = 0; rt < RT; ++rt) add4(s, sb[((size_t)img * RT + rt) * N + i]);
        reinterpret_cast<float4*>(d_b)[(size_t)img * N + i] = s;
    }
}

}  // namespace

extern "C" size_t gnms_iou2d_backward_workspace_bytes(int B, int M, int N) {
    if (B <= 0 || M <= 0 || N <= 0) return 0;
    const SlabPlan s = plan_for(B, M, N);
    return s.a_bytes + s.b_bytes;
}

extern "C" int gnms_iou2d_backward(const float* boxes_a, const float* boxes_b, const float* grad, int B, int M, int N, int64_t ld,
                                   float* d_boxes_a, float* d_boxes_b, void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && M >= 0 && N >= 0, "gnms_iou2d_backward: negative size (B=%d M=%d N=%d)", B, M, N);
    GNMS_CHECK_ARG(d_boxes_a || d_boxes_b, "gnms_iou2d_backward: both outputs are NULL");
    const bool self = boxes_b == nullptr;
    if (self) {
        GNMS_CHECK_ARG(M == N, "gnms_iou2d_backward: boxes_b is NULL (boxes_a on both sides) but M (%d) != N (%d)", M, N);
        GNMS_CHECK_ARG(d_boxes_a && !d_boxes_b, "gnms_iou2d_backward: boxes_b is NULL: both roles are summed into d_boxes_a, d_boxes_b must be NULL");
    }
    GNMS_CHECK_ARG(ld >= N, "gnms_iou2d_backward: ld (%lld) < N (%d)", (long long)ld, N);
    GNMS_CHECK_ARG(((uintptr_t)d_boxes_a % 16 == 0) && ((uintptr_t)d_boxes_b % 16 == 0), "gnms_iou2d_backward: outputs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return GNMS_OK;
    if (M == 0 || N == 0) {                                           // no pair: every element that exists is written, with 0
        if (d_boxes_a && M > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_boxes_a, 0, sizeof(float) * 4 * (size_t)B * M, st));
        if (d_boxes_b && N > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_boxes_b, 0, sizeof(float) * 4 * (size_t)B * N, st));
        return GNMS_OK;
    }
    GNMS_CHECK_ARG(boxes_a && grad, "gnms_iou2d_backward: null boxes_a / grad");
    GNMS_CHECK_ARG(((uintptr_t)boxes_a % 16 == 0) && ((uintptr_t)boxes_b % 16 == 0), "gnms_iou2d_backward: boxes must be 16-byte aligned");
    GNMS_CHECK_ARG(workspace != nullptr, "gnms_iou2d_backward: workspace is NULL");
    GNMS_CHECK_ARG((uintptr_t)workspace % 256 == 0, "gnms_iou2d_backward: workspace must be 256-byte aligned");
    const SlabPlan s = plan_for(B, M, N);
    if (workspace_bytes < s.a_bytes + s.b_bytes) {
        gnms_set_error("gnms_iou2d_backward: workspace too small (%zu < %zu)", workspace_bytes, s.a_bytes + s.b_bytes);
        return GNMS_ERR_WORKSPACE;
    }
    float* slab_a = reinterpret_cast<float*>(workspace);
    float* slab_b = reinterpret_cast<float*>(static_cast<char*>(workspace) + s.a_bytes);
    const bool want_a = d_boxes_a != nullptr, want_b = self || d_boxes_b != nullptr;
    const long units = (long)B * s.RT * s.CT;
    const dim3 grid((unsigned)((units + kUnitsPerWG - 1) / kUnitsPerWG));
    const float* bb = self ? boxes_a : boxes_b;
    const int vec = (ld % 4 == 0) && ((uintptr_t)grad % 16 == 0);   // 16-byte loads of the cotangent
#define GNMS_IOU_BWD(WA, WB) \
    iou2d_backward_kernel<WA, WB><<<grid, 64 * kUnitsPerWG, 0, st>>>(boxes_a, bb, grad, M, N, (long)ld, vec, s.rc, s.RT, s.CT, units, slab_a, slab_b)
    if (want_a && want_b) GNMS_IOU_BWD(true, true);
    else if (want_a) GNMS_IOU_BWD(true, false);
    else GNMS_IOU_BWD(false, true);
#undef GNMS_IOU_BWD
    GNMS_CHECK_LAUNCH();
    iou2d_backward_reduce_kernel<<<dim3(gnms_div_up(M > N ? M : N, 256), B, self ? 1 : 2), 256, 0, st>>>(slab_a, slab_b, M, N, s.CT, s.RT, d_boxes_a,
                                                                                                         d_boxes_b, self ? 1 : 0);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
