// pair_grad_walker.h -- the cotangent of a pairwise overlap matrix contracted with d overlap / d box, for any geometry G (DESIGN 3.23,
// 3.24): the walker kernel, the slab reduce and the host code of gnms_iou2d_backward (iou_backward.hip) and gnms_iou3d_backward
// (iou3d_backward.hip).  Each of those units instantiates the kernels for its own G and nothing else.
//
//   d_a[b][i] = sum_j grad[b][i][j] * d f(a_i, b_j)/d a_i          d_b[b][j] = sum_i grad[b][i][j] * d f(a_i, b_j)/d b_j
//
// One WAVE owns a unit of (rc x 32) rows x (64 x G::kSubTiles) columns and walks it in chunks of 32 rows x 64 columns.  A chunk's
// cotangents are read from memory ONCE (16-byte loads where ld and the pointer allow, else lane = column) into the wave's own 8 KiB of
// LDS, and used twice:
//   column pass: lane = column, the 32 rows one after the other   -> G::kAcc accumulators per column, kept in registers down the unit
//   row pass   : lane = (row, column half), 32 columns each       -> G::kAcc accumulators per row, the halves added (low + high)
// Both sums run in a fixed order.  Units meet only in memory: a unit stores its row sums into slab_a[column tile] and its column sums
// into slab_b[row tile], and pair_grad_reduce_kernel adds the slabs in tile order -- no float atomics, the same bits every run -- and
// hands a box's sum to G::finish.  A chunk, and inside it a wave-step, whose 64 cotangents are all zero skips the arithmetic: the
// masked-group layer's matrix gradient has one non-zero per row, and the walker then runs at the speed of the read.
//
// A geometry G is a struct of constants and __device__ __forceinline__ statics:
//   kAcc, kSubTiles       accumulators per box (4 coordinates / 6 extents); 64-column sub-tiles per unit (kSubTiles * kAcc column sums a lane)
//   kWalkFloats, kStash4  floats per box of the arrays the walker reads; float4s per column of the wave's LDS column stash
//   kBoxFloats, kAlign16  floats per box of the entry's inputs and outputs (4 / 7); whether those must be 16-byte aligned; kWhat names them
//   Box                   what a lane holds for a box;  load(array, index)
//   stash / unstash       to and from the column stash;  bcast(box, lane)
//   Pair, pair(a, b)      a: the row box, b: the column box;  add_grad(s, o, pair, g, acc): acc += g * d f / d s, o the other box
//   store_slab / add_slab a box's kAcc sums to and from a slab
//   finish                what the reduce does with a box's sum;  Sums: the struct that holds these three (G, or a base of several G)
//   records_bytes / prepare (host)  workspace in front of the slabs and the launches that fill it with the arrays the walker reads
// How a G passes the state (by value / by reference, an address / an index) decides the walker's register allocation: see the note at
// Iou3dCuboids (iou3d_backward.hip) and LABNOTES R17.2 before tidying one.
#pragma once
#include "gnms_common.h"

namespace gnms_pair_grad {

constexpr int kChunkRows = 32;
constexpr int kSubCols = 64;
constexpr int kUnitsPerWG = 4;                   // waves of a workgroup; they share nothing

// 32-row chunks per unit: 8 (256 rows) unless that leaves the chip short of waves.  A wave loads a chunk, then works on it, so the read
// is hidden by OTHER waves: 12 resident per CU (__launch_bounds__(256, 3)) and a few rounds of them -- 8192 units -- before the units
// grow.  2D, B = 8, N = 4096: 2 chunks per unit, 33 MB of column slabs beside the 512 MB matrix.
// What the compiler reports (tools/kernel_resources.sh; VGPRs for WANT_A and WANT_B / WANT_A / WANT_B, 3 waves per SIMD, no scratch):
//   2D 163 / 143 / 144, LDS 36864 / 36864 / 32768 B;   3D 161-164 / 139-145 / 137-150, LDS 40960 / 40960 / 32768 B.
// The 2D walker is one small change away from spilling: with the lane-per-column pointer formed from the unclamped column it takes
// 168 VGPRs and 104 / 20 / 28 B of scratch per lane (LABNOTES R17).  Look at the rows again after any change to the kernel or to a G.
inline int chunks_per_unit(int B, int M, int N, int unit_cols) {
    int rc = 8;
    while (rc > 1 && (long long)B * gnms_div_up(M, kChunkRows * rc) * gnms_div_up(N, unit_cols) < 8192) rc >>= 1;
    return rc;
}

struct SlabPlan {
    int rc, RT, CT;
    size_t a_bytes, b_bytes;
};
template <class G>
SlabPlan plan_for(int B, int M, int N) {
    SlabPlan s;
    s.rc = chunks_per_unit(B, M, N, kSubCols * G::kSubTiles);
    s.RT = gnms_div_up(M, kChunkRows * s.rc);
    s.CT = gnms_div_up(N, kSubCols * G::kSubTiles);
    s.a_bytes = gnms_align_up((size_t)B * s.CT * M * G::kAcc * sizeof(float), 256);
    s.b_bytes = gnms_align_up((size_t)B * s.RT * N * G::kAcc * sizeof(float), 256);
    return s;
}

// orders the wave's own LDS stores and loads (the tile is private to the wave: no workgroup barrier anywhere in this kernel)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

template <class G, bool WANT_A, bool WANT_B>
__global__ __launch_bounds__(256, 3) void pair_grad_walker_kernel(const float* __restrict__ A, const float* __restrict__ Bx,
                                                               const float* __restrict__ grad, int M, int N, long ld, int vec, int rc, int RT,
                                                               int CT, long units, float* __restrict__ slab_a, float* __restrict__ slab_b) {
    using Box = typename G::Box;
    constexpr int kUnitCols = kSubCols * G::kSubTiles;
    __shared__ float tiles[kUnitsPerWG][kChunkRows * kSubCols];
    __shared__ float4 stashes[kUnitsPerWG][G::kStash4 * kSubCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long unit = (long)blockIdx.x * kUnitsPerWG + wave;
    if (unit >= units) return;
    const int ct = (int)(unit % CT), rt = (int)((unit / CT) % RT), img = (int)(unit / ((long)CT * RT));
    const float* a = A + (size_t)img * M * G::kWalkFloats;
    const float* bx = Bx + (size_t)img * N * G::kWalkFloats;
    const float* g = grad + (size_t)img * M * ld;
    float* t = tiles[wave];
    float4* cb = stashes[wave];
    const int row_begin = rt * rc * kChunkRows;
    const int row_end = min(M, row_begin + rc * kChunkRows);
    const int col0 = ct * kUnitCols;
    const int lrow = lane & 31, half = lane >> 5;

    float accb[G::kSubTiles][G::kAcc];
#pragma unroll
    for (int cs = 0; cs < G::kSubTiles; ++cs)
#pragma unroll
        for (int k = 0; k < G::kAcc; ++k) accb[cs][k] = 0.0f;

    for (int r0 = row_begin; r0 < row_end; r0 += kChunkRows) {
        const int myrow = r0 + lrow;                                  // lanes r and r + 32 hold row r0 + r
        const Box ra = G::load(a, (size_t)min(myrow, M - 1));
        float acca[G::kAcc];
#pragma unroll
        for (int k = 0; k < G::kAcc; ++k) acca[k] = 0.0f;
#pragma unroll
        for (int cs = 0; cs < G::kSubTiles; ++cs) {
            const int c0 = col0 + cs * kSubCols;
            if (c0 < N) {
                const int col = c0 + lane;
                const Box cbox = G::load(bx, (size_t)min(col, N - 1));
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
                    const float* gp = g + (size_t)r0 * ld + min(col, N - 1);          // (never past the row, loaded or not)
#pragma unroll 8
                    for (int r = 0; r < kChunkRows; ++r) {
                        const float v = (r0 + r < row_end && col < N) ? gp[(size_t)r * ld] : 0.0f;
                        nz = nz || v != 0.0f;
                        t[r * kSubCols + (lane ^ r)] = v;
                    }
                }
                if (__ballot(nz) != 0ull) {
                    if (WANT_A) G::stash(cb + G::kStash4 * lane, cbox);
                    wave_lds_fence();
                    if (WANT_B) {
                        for (int r = 0; r < kChunkRows; ++r) {
                            const float v = t[r * kSubCols + (lane ^ r)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const Box rb = G::bcast(ra, r);
                            const typename G::Pair p = G::pair(rb, cbox);
                            G::add_grad(cbox, rb, p, v, accb[cs]);
                        }
                    }
                    if (WANT_A) {
                        for (int j = 0; j < 32; ++j) {
                            const int c = 32 * half + j;
                            const float v = t[lrow * kSubCols + (c ^ lrow)];
                            if (__ballot(v != 0.0f) == 0ull) continue;
                            const Box ob = G::unstash(cb + G::kStash4 * c);
                            const typename G::Pair p = G::pair(ra, ob);
                            G::add_grad(ra, ob, p, v, acca);
                        }
                    }
                    wave_lds_fence();                                 // the next chunk's stores come after these loads
                }
            }
        }
        if (WANT_A) {
#pragma unroll
            for (int k = 0; k < G::kAcc; ++k) acca[k] = acca[k] + __shfl_down(acca[k], 32);     // columns 0..31 + columns 32..63
            if (half == 0 && myrow < row_end) G::store_slab(slab_a, ((size_t)img * CT + ct) * M + myrow, acca);
        }
    }
    if (WANT_B) {
#pragma unroll
        for (int cs = 0; cs < G::kSubTiles; ++cs) {
            const int col = col0 + cs * kSubCols + lane;
            if (col < N) G::store_slab(slab_b, ((size_t)img * RT + rt) * N + col, accb[cs]);
        }
    }
}

// blockIdx.z = 0: the sums of a_i = slab_a[0][i] + slab_a[1][i] + ... (then, self: + slab_b[0][i] + ...); 1: those of b_j from slab_b.
// Then G::finish on the box's own input.
template <class G>
__global__ __launch_bounds__(256) void pair_grad_reduce_kernel(const float* __restrict__ slab_a, const float* __restrict__ slab_b,
                                                               const float* __restrict__ in_a, const float* __restrict__ in_b, int M, int N,
                                                               int CT, int RT, float* __restrict__ d_a, float* __restrict__ d_b, int self) {
    const int img = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float s[G::kAcc];
#pragma unroll
    for (int k = 0; k < G::kAcc; ++k) s[k] = 0.0f;
    if (blockIdx.z == 0) {
        if (!d_a || i >= M) return;
        for (int ct = 0; ct < CT; ++ct) G::add_slab(s, slab_a, ((size_t)img * CT + ct) * M + i);
        if (self)
            for (int rt = 0; rt < RT; ++rt) G::add_slab(s, slab_b, ((size_t)img * RT + rt) * N + i);
        G::finish(in_a, d_a, (size_t)img * M + i, s);
    } else {
        if (!d_b || i >= N) return;
        for (int rt = 0; rt < RT; ++rt) G::add_slab(s, slab_b, ((size_t)img * RT + rt) * N + i);
        G::finish(in_b, d_b, (size_t)img * N + i, s);
    }
}

template <class G>
size_t workspace_bytes(int B, int M, int N, bool self) {
    const SlabPlan s = plan_for<G>(B, M, N);
    return G::records_bytes((long)B * M) + (self ? 0 : G::records_bytes((long)B * N)) + s.a_bytes + s.b_bytes;
}

// the body of an extern "C" backward entry `name`: argument checks, workspace split, G::prepare, walker, reduce
template <class G>
int backward(const char* name, const float* in_a, const float* in_b, const float* grad, int B, int M, int N, int64_t ld, float* d_a, float* d_b,
             void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* w = G::kWhat;
    GNMS_CHECK_ARG(B >= 0 && M >= 0 && N >= 0, "%s: negative size (B=%d M=%d N=%d)", name, B, M, N);
    GNMS_CHECK_ARG(d_a || d_b, "%s: both outputs are NULL", name);
    const bool self = in_b == nullptr;
    if (self) {
        GNMS_CHECK_ARG(M == N, "%s: %s_b is NULL (%s_a on both sides) but M (%d) != N (%d)", name, w, w, M, N);
        GNMS_CHECK_ARG(d_a && !d_b, "%s: %s_b is NULL: both roles are summed into d_%s_a, d_%s_b must be NULL", name, w, w, w);
    }
    GNMS_CHECK_ARG(ld >= N, "%s: ld (%lld) < N (%d)", name, (long long)ld, N);
    if (G::kAlign16) GNMS_CHECK_ARG(((uintptr_t)d_a % 16 == 0) && ((uintptr_t)d_b % 16 == 0), "%s: outputs must be 16-byte aligned", name);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return GNMS_OK;
    if (M == 0 || N == 0) {                                           // no pair: every element that exists is written, with 0
        if (d_a && M > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_a, 0, sizeof(float) * G::kBoxFloats * (size_t)B * M, st));
        if (d_b && N > 0) GNMS_CHECK_HIP(hipMemsetAsync(d_b, 0, sizeof(float) * G::kBoxFloats * (size_t)B * N, st));
        return GNMS_OK;
    }
    GNMS_CHECK_ARG(in_a && grad, "%s: null %s_a / grad", name, w);
    if (G::kAlign16) GNMS_CHECK_ARG(((uintptr_t)in_a % 16 == 0) && ((uintptr_t)in_b % 16 == 0), "%s: %s must be 16-byte aligned", name, w);
    GNMS_CHECK_ARG(workspace != nullptr, "%s: workspace is NULL", name);
    GNMS_CHECK_ARG((uintptr_t)workspace % 256 == 0, "%s: workspace must be 256-byte aligned", name);
    const SlabPlan s = plan_for<G>(B, M, N);
    const size_t rec_a = G::records_bytes((long)B * M), rec_b = self ? 0 : G::records_bytes((long)B * N);
    if (workspace_bytes_given < rec_a + rec_b + s.a_bytes + s.b_bytes) {
        gnms_set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes_given, workspace_bytes<G>(B, M, N, false));   // (what the query returns)
        return GNMS_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    float* slab_a = reinterpret_cast<float*>(ws + rec_a + rec_b);
    float* slab_b = reinterpret_cast<float*>(ws + rec_a + rec_b + s.a_bytes);
    // what the walker reads: the inputs themselves, or G's records of them in front of the slabs
    const float* walk_a = in_a;
    const float* walk_b = self ? in_a : in_b;
    if (rec_a) {
        int rc;
        if ((rc = G::prepare(in_a, (long)B * M, reinterpret_cast<float*>(ws), st))) return rc;
        if (!self && (rc = G::prepare(in_b, (long)B * N, reinterpret_cast<float*>(ws + rec_a), st))) return rc;
        walk_a = reinterpret_cast<const float*>(ws);
        walk_b = self ? walk_a : reinterpret_cast<const float*>(ws + rec_a);
    }
    const bool want_a = d_a != nullptr, want_b = self || d_b != nullptr;
    const long units = (long)B * s.RT * s.CT;
    const dim3 grid((unsigned)((units + kUnitsPerWG - 1) / kUnitsPerWG));
    const int vec = (ld % 4 == 0) && ((uintptr_t)grad % 16 == 0);   // 16-byte loads of the cotangent
#define GNMS_PAIR_GRAD_WALK(WA, WB) \
    pair_grad_walker_kernel<G, WA, WB><<<grid, 64 * kUnitsPerWG, 0, st>>>(walk_a, walk_b, grad, M, N, (long)ld, vec, s.rc, s.RT, s.CT, units, slab_a, slab_b)
    if (want_a && want_b) GNMS_PAIR_GRAD_WALK(true, true);
    else if (want_a) GNMS_PAIR_GRAD_WALK(true, false);
    else GNMS_PAIR_GRAD_WALK(false, true);
#undef GNMS_PAIR_GRAD_WALK
    GNMS_CHECK_LAUNCH();
    pair_grad_reduce_kernel<typename G::Sums><<<dim3(gnms_div_up(M > N ? M : N, 256), B, self ? 1 : 2), 256, 0, st>>>(
        slab_a, slab_b, in_a, self ? in_a : in_b, M, N, s.CT, s.RT, d_a, d_b, self ? 1 : 0);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

}  // namespace gnms_pair_grad
