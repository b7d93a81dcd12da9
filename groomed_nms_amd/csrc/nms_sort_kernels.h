// nms_sort_kernels.h -- K1 of the GrooMeD-NMS layer: the stable descending argsort of the scores and, on the from-boxes paths, the
// column order of the boxes (by x centre), as one workgroup per image (sort_scores_kernel), runs + merge, ranked runs, by histogram, or by
// counting.  Everything here is a template or a __device__ body: a translation unit that includes this header (soft_sort.hip borrows
// sort_scores_kernel<E>) gets only the kernels it instantiates.  The non-template wrappers over sort_runs_body, sort_ranked_runs_body and
// sort_hist_rank_body, which only the layer launches, are in nms_kernels.h.
#pragma once
#include "gnms_device.h"
#include "sort_bins.h"

namespace gnms {
namespace {   // internal linkage: the header is included by several translation units

// ------------------------------------------------------------------------------------------------
// K1: stable descending argsort of the scores (lib/groomed_nms.py:41; get_groups :213)
// ------------------------------------------------------------------------------------------------
// Second, independent sort of the from-boxes path: the boxes by ascending x centre (NaN last).  bitmask_boxes_kernel walks
// its COLUMNS in this order, so that the 256 columns of a wave tile are spatial neighbours and the rows that cannot touch
// their hull are skipped.  Thread t owns elements t*E .. t*E+E-1; `keys` = P 64-bit LDS slots.
// A box the packed intersection of bitmask_boxes_body may see: finite coordinates, no negative zero, x2 >= x1, y2 >= y1
__device__ __forceinline__ bool box_orders_plainly(const float4 v) {
    auto fine = [](float c) { const unsigned u = __float_as_uint(c); return u != 0x80000000u && (u & 0x7fffffffu) < 0x7f800000u; };
    return fine(v.x) && fine(v.y) && fine(v.z) && fine(v.w) && v.z >= v.x && v.w >= v.y;
}

// Column order of the 3D bit-matrix kernel (bitmask_rec3d_slots_kernel): the cuboids arrive as pseudo boxes (x0, lx, x1, z0 + z1) and
// are ordered by (z band, x centre) -- `mode3d` equal-width bands over the image's range of z0 + z1 -- so that 64 consecutive columns
// (one SLOT of a wave tile) are a compact patch in x AND z and the rows far from it in either direction are skipped.  mode3d = 0: plain
// 2D boxes by x centre; 1: cuboids, one band.  Key = band << 60 | x key << 28 | input index (N <= 16384): distinct, NaN x last.
constexpr unsigned kColIdxMask = 0x0fffffffu;
__device__ __forceinline__ unsigned column_band(const float4 v, int nbands, float zlo, float zscale) {
    if (nbands <= 1) return 0u;
    const float f = (v.w - zlo) * zscale;
    return (f == f) ? (unsigned)fminf(fmaxf(f, 0.0f), (float)(nbands - 1)) : (unsigned)(nbands - 1);
}
__device__ __forceinline__ u64 column_key(const float4 v, int i, int nbands, float zlo, float zscale) {
    return ((u64)column_band(v, nbands, zlo, zscale) << 60) | ((u64)(~gnms_desc_key(v.x + v.z)) << 28) | (unsigned)i;
}
// range of z0 + z1 over the image's finite pseudo boxes -> (zlo, nbands / (zhi - zlo)); every thread of the workgroup returns the same pair
// (min / max do not depend on the order), so every workgroup of an image bands alike
__device__ __forceinline__ void block_z_bands(const float4* __restrict__ bx, int n, int nbands, float* zlo_out, float* zscale_out) {
    __shared__ float zred[2][16];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float z = bx[i].w;
        if (fabsf(z) < INFINITY) { lo = fminf(lo, z); hi = fmaxf(hi, z); }
    }
    lo = gnms_wave_min_f(lo); hi = gnms_wave_max_f(hi);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { zred[0][wave] = lo; zred[1][wave] = hi; }
    __syncthreads();
    lo = INFINITY; hi = -INFINITY;
    for (int w = 0; w < nw; ++w) { lo = fminf(lo, zred[0][w]); hi = fmaxf(hi, zred[1][w]); }
    const float span = hi - lo;
    *zlo_out = lo;
    *zscale_out = (span > 0.0f && span < INFINITY) ? (float)nbands / span : 0.0f;
    __syncthreads();
}
// what the column sort leaves behind for rank `k` of its order: the input index, the (pseudo) box, and for cuboids the record
__device__ __forceinline__ void column_store(const ImgPtrs& I, int k, int idx, const float4 v, int mode3d) {
    I.xidx[k] = idx;
    I.xbox[k] = v;
    if (mode3d) {
        const float4* s = reinterpret_cast<const float4*>(I.rec) + (size_t)idx * 3;
        float4* d = reinterpret_cast<float4*>(I.xrec) + (size_t)k * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
}

template <int E>
__device__ __forceinline__ void sort_boxes_by_x(const float* __restrict__ boxes, int n, const ImgPtrs& I, u64* keys, int P, int mode3d = 0) {
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    float zlo = 0.0f, zscale = 0.0f;
    if (mode3d > 1) block_z_bands(bx, n, mode3d, &zlo, &zscale);
    u64 r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = threadIdx.x * E + e;
        r[e] = ~0ull;
        if (i < n) r[e] = column_key(bx[i], i, mode3d, zlo, zscale);
    }
    block_sort<E, u64>(r, keys, P);
    bool plain = true;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int idx = (int)((unsigned)keys[k] & kColIdxMask);
        const float4 v = bx[idx];
        column_store(I, k, idx, v, mode3d);
        plain = plain && box_orders_plainly(v);
    }
    const int all_plain = __syncthreads_and(plain);
    if (threadIdx.x == 0) I.misc[6] = all_plain ? 0 : 1;              // bitmask_boxes_body: the packed intersection needs plain boxes
}

template <int E>
__global__ __launch_bounds__(1024) void sort_scores_kernel(const float* __restrict__ scores, int N, const int* __restrict__ counts,
                                                           char* ws, gnms_ws_layout L, int P, long long* __restrict__ order_out,
                                                           const float* __restrict__ boxes, int mode3d) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    const int b = blockIdx.x;
    const int n = gnms_count(counts, b, N);
    const float* s = scores + (size_t)b * N;
    ImgPtrs I = img_ptrs(ws, L, b);
    if (blockIdx.y == 1) {                      // from-boxes path only: grid (B, 2)
        sort_boxes_by_x<E>(boxes + (size_t)b * N * 4, n, I, keys, P, mode3d);
        return;
    }
    u64 r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = threadIdx.x * E + e;
        r[e] = (i < n) ? (((u64)gnms_desc_key(s[i]) << 32) | (unsigned)i) : ~0ull;
    }
    block_sort<E, u64>(r, keys, P);
    int same = 1;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        int idx = k;                  // padding ranks map to themselves
        float v = 0.0f;
        if (k < n) { idx = (int)(keys[k] & 0xffffffffu); v = s[idx]; }
        same &= (idx == k);
        I.order[k] = idx;
        I.rankof[idx] = k;            // order is a permutation of [0,N) (identity on the padding)
        I.sscore[k] = v;
        if (boxes && k < n) I.rbox[k] = reinterpret_cast<const float4*>(boxes)[(size_t)b * N + idx];   // (the from-boxes layer: row boxes of the bit matrix)
        if (order_out) order_out[(size_t)b * N + k] = idx;
    }
    // misc[2] = 1 when the scores came in already sorted (both reference call sites do that: lib/loss/rpn_3d.py:731-737,
    // lib/rpn_util.py:1258-1266): rank == input index, so the bit-matrix kernel can skip the half of the matrix that no
    // leader can reach and needs no scatter.
    const int all_same = __syncthreads_and(same);
    if (threadIdx.x < 8 && !(boxes && threadIdx.x == 6)) I.misc[threadIdx.x] = (threadIdx.x == 2) ? all_same : 0;   // ([6]: the x sort's)
    if (threadIdx.x == 8) I.misc[8] = gnms_next_epoch(I.misc[8]);                   // the workspace's call counter (leaders_sb_body's hand-off tag)
    for (int i = threadIdx.x; i < 17 * 32; i += blockDim.x) I.gran[i] = 0ull;   // (and no granule of this workspace carries a tag yet)
}

// ------------------------------------------------------------------------------------------------
// K1 as runs + merge: the same two sorts (scores descending; boxes by x centre) spread over R = P/1024 workgroups per image.  The route of
// N > 4096; up to 2048 keys the counting sort further down took over in round 5, and 2048 < N <= 4096 the ranked runs behind these two in
// round 8 (launch_sorts in nms_layer.hip has the table; GNMS_RANK_SORT=0 brings that range back here).
//   sort_runs_kernel  every workgroup sorts one run of 1024 keys in LDS (block_sort<1>) and parks it in global scratch
//                      (the bit-matrix region W: nothing lives there before K2);
//   sort_merge_kernel  every workgroup loads ALL runs of its image into LDS and ranks its own 1024 keys: final position =
//                      own position + sum over the other runs of (number of keys below mine), R-1 branch-free binary searches
//                      that advance in lock step (their LDS reads overlap).  Keys are distinct (index in the low word).
// One workgroup per image needs 23 us at N=4096 and 103 us at N=16384 on its single CU; this needs about 10 / 20 us.
// role (blockIdx.z): 0 = scores, 1 = boxes by x centre (from-boxes path).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 sort_key_of(int role, const float* __restrict__ scores_img, const float* __restrict__ boxes_img, int i,
                                           int nbands, float zlo, float zscale) {
    if (role == 0) return ((u64)gnms_desc_key(scores_img[i]) << 32) | (unsigned)i;
    return column_key(reinterpret_cast<const float4*>(boxes_img)[i], i, nbands, zlo, zscale);
}

// (run r of image b, role)
__device__ __forceinline__ void sort_runs_body(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                               const int* __restrict__ counts, char* ws, gnms_ws_layout L, int P, const int r, const int b,
                                               const int role, const int mode3d = 0) {
    __shared__ u64 keys[1024];
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int i = r * 1024 + (int)threadIdx.x;
    float zlo = 0.0f, zscale = 0.0f;
    if (role == 1 && mode3d > 1) block_z_bands(reinterpret_cast<const float4*>(boxes + (size_t)b * N * 4), n, mode3d, &zlo, &zscale);
    u64 k[1];
    k[0] = (i < n) ? sort_key_of(role, scores + (size_t)b * N, boxes ? boxes + (size_t)b * N * 4 : nullptr, i, mode3d, zlo, zscale) : ~0ull;
    block_sort<1, u64>(k, keys, 1024);
    I.W[(size_t)role * P + i] = k[0];
    if (r == 0 && role == 0 && threadIdx.x < 8) I.misc[threadIdx.x] = (threadIdx.x == 2) ? 1 : 0;   // [2] = "already sorted", cleared below
    if (r == 0 && role == 0 && threadIdx.x == 8) I.misc[8] = gnms_next_epoch(I.misc[8]);   // the workspace's call counter (leaders_sb_body's hand-off tag)
    if (r == 0 && role == 0 && threadIdx.x < 17 * 32) I.gran[threadIdx.x] = 0ull;   // (and no granule of this workspace carries a tag yet)
}

template <int R>
__device__ __forceinline__ void sort_merge_body(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                const int* __restrict__ counts, char* ws, gnms_ws_layout L, long long* __restrict__ order_out,
                                                const int r, const int b, const int role, const int mode3d = 0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* all = reinterpret_cast<u64*>(smem);                          // [R][1024]
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int t = threadIdx.x;
    const u64* runs = I.W + (size_t)role * (R * 1024);
#pragma unroll
    for (int q = 0; q < R; ++q)
        all[q * 1024 + t] = runs[q * 1024 + t];
    __syncthreads();
    const u64 mine = all[r * 1024 + t];
    int same = 1;
    if (mine != ~0ull) {
        // what leaves with the key -- its score, its box -- is fetched by INPUT index, known before the searches: requested here, the round
        // trip runs under them (round 6: behind the rank it was one more exposed memory latency at the end of every workgroup)
        const int idx = (int)((unsigned)mine & (role == 0 ? 0xffffffffu : kColIdxMask));
        float sv = 0.0f;
        float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (role == 0) sv = scores[(size_t)b * N + idx];
        if (boxes) bv = reinterpret_cast<const float4*>(boxes)[(size_t)b * N + idx];
        int pos[R];
#pragma unroll
        for (int q = 0; q < R; ++q) pos[q] = 0;
#pragma unroll
        for (int h = 512; h >= 1; h >>= 1) {
#pragma unroll
            for (int q = 0; q < R; ++q) pos[q] += (all[q * 1024 + pos[q] + h - 1] < mine) ? h : 0;
        }
        int rank = 0;
#pragma unroll
        for (int q = 0; q < R; ++q) rank += (q == r) ? t : pos[q] + ((all[q * 1024 + pos[q]] < mine) ? 1 : 0);
        if (role == 0) {
            same = (idx == rank);
            I.order[rank] = idx;
            I.rankof[idx] = rank;
            I.sscore[rank] = sv;
            if (boxes) I.rbox[rank] = bv;                             // (the from-boxes layer: row boxes of the bit matrix)
            if (order_out) order_out[(size_t)b * N + rank] = idx;
        } else {
            column_store(I, rank, idx, bv, mode3d);
            same = box_orders_plainly(bv);                            // (role 1: "every box of this run is plain")
        }
    }
    if (role == 1 && !__syncthreads_and(same) && t == 0) I.misc[6] = 1;   // (zeroed by sort_runs_body, a launch earlier; every writer stores 1)
    if (role == 0) {
        // padding ranks map to themselves (order is a permutation of [0, N))
        for (int k = n + r * 1024 + t; k < N; k += R * 1024) {
            I.order[k] = k; I.rankof[k] = k; I.sscore[k] = 0.0f;
            if (order_out) order_out[(size_t)b * N + k] = k;
        }
        if (!__syncthreads_and(same) && t == 0) I.misc[2] = 0;        // (every writer stores 0)
    }
}

template <int R>
__global__ __launch_bounds__(1024) void sort_merge_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                          const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                          long long* __restrict__ order_out, int mode3d) {
    sort_merge_body<R>(scores, boxes, N, counts, ws, L, order_out, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, mode3d);
}

// ------------------------------------------------------------------------------------------------
// K1 for 2048 < N <= 4096 (round 8): runs AND ranks in ONE launch, no workgroup waiting for another.  Runs + merge cost 8.1 + 6.4 us and a
// launch boundary at B = 8 on 64 workgroups each, the keys going through HBM scratch in between.  Here workgroup (r, image, role) of
// 16 builds ALL 4096 keys of its image and role (thread t: keys 4t .. 4t+3), each of its 16 waves sorts its own 256 keys in registers
// (phase 1 of block_sort<4>: no barrier inside), the 16 sorted runs go into LDS, and the workgroup ranks the 256 keys of run r against all
// runs: thread (key, quarter) searches the four runs of its quarter in lock step, the four partial counts meet in LDS.  Every image's
// run sort is repeated 16 times -- on CUs that stood idle -- and that is what removes the second launch, the scratch and every hand-off.
// 16 * B * roles workgroups: 256 at B = 8 with boxes; taken while that is one round of the machine (launch_sorts).  The flags are decided by workgroup 0 of each role alone, on the keys it holds
// (as sort_count_body does): no flag depends on an earlier launch.
// ------------------------------------------------------------------------------------------------
constexpr int kRankRuns = 16;            // waves per workgroup = runs per image = workgroups per image and role
constexpr int kRankRunKeys = 256;        // keys per run (E = 4 per lane)

// lane ^ m of a 32-bit value, m a compile-time constant after unrolling: DPP where one exists (quad_perm for 1 and 2, row_ror:8 for 8, the two
// halves of 4 as row_ror:12 into banks 0, 2 and row_ror:4 into banks 1, 3), ds_bpermute for 16 and 32.  18 of the run sort's 21 shuffle stages
// are DPP that way; with ds_bpermute for all of them the launch took 14.6 us instead of 11.5 at B = 8 (LABNOTES R8.2)
__device__ __forceinline__ unsigned xor_lanes32(unsigned v, int m) {
    switch (m) {
        case 1: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm:[1,0,3,2]
        case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm:[2,3,0,1]
        case 4: {
            const int a = __builtin_amdgcn_update_dpp(0, (int)v, 0x12C, 0xF, 0x5, false);         // row_ror:12 = lane + 4 -> lanes with bit 2 clear
            return (unsigned)__builtin_amdgcn_update_dpp(a, (int)v, 0x124, 0xF, 0xA, false);      // row_ror:4  = lane - 4 -> lanes with bit 2 set
        }
        case 8: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);   // row_ror:8
        default: break;
    }
    return __shfl_xor(v, m, 64);
}
__device__ __forceinline__ u64 xor_lanes(u64 v, int m) {
    return ((u64)xor_lanes32((unsigned)(v >> 32), m) << 32) | xor_lanes32((unsigned)(v & 0xffffffffu), m);
}

// every wave sorts the 256 keys of its lanes' r[0..3] ascending (lane l ends with positions 4l .. 4l+3 of the run): the network of
// block_sort's phase 1 for E = 4, fully unrolled so that every shuffle distance is a constant
__device__ __forceinline__ void wave_sort_256(u64 (&r)[4]) {
    const int i0 = ((int)threadIdx.x & 63) * 4;
#pragma unroll
    for (int k = 2; k <= kRankRunKeys; k <<= 1) {
        const int kd = (k == kRankRunKeys) ? 0 : k;
#pragma unroll
        for (int j = k >> 1; j >= 4; j >>= 1) {
            const bool keepmin = ((i0 & kd) == 0) == ((i0 & j) == 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u64 o = xor_lanes(r[e], j / 4);
                r[e] = ((o < r[e]) == keepmin) ? o : r[e];
            }
        }
#pragma unroll
        for (int jj = 2; jj >= 1; jj >>= 1) {
            if (jj < k) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((e & jj) == 0) {
                        const bool up = ((i0 + e) & kd) == 0;
                        const u64 a = r[e], b = r[e | jj];
                        if ((a > b) == up) { r[e] = b; r[e | jj] = a; }
                    }
                }
            }
        }
    }
}

// developer (tools/sort_ticks.py, timing build): the clock at the phase boundaries of wave 0 and wave 15 of workgroup 8 of image 0, per role,
// the differences summed into xsol behind the bit-matrix kernel's slots.  Every tick drains the wave's memory operations first, so that a
// phase is charged with the loads it issued.  path: 0 = sort_ranked_runs_kernel, 1 = sort_hist_rank_kernel by histogram, 2 = its fallback
struct SortTicks {
#ifdef GNMS_TIMING
    long long v[10];
    int n = 0;
    __device__ __forceinline__ void tick() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0);
        v[n++] = (long long)__builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void flush(const ImgPtrs& I, int b, int r, int role, int path) const {
        if (b != 0 || r != 8 || (threadIdx.x != 0 && threadIdx.x != 960)) return;
        long long* o = reinterpret_cast<long long*>(I.xsol) + 600 + path * 64 + role * 32 + (threadIdx.x ? 16 : 0);
        for (int q = 1; q < n; ++q) o[q] += v[q] - v[q - 1];
    }
#else
    __device__ __forceinline__ void tick() {}
    __device__ __forceinline__ void flush(const ImgPtrs&, int, int, int, int) const {}
#endif
};

// Thread t builds four keys of its image and role (padding ~0: behind everything) and keeps the value each is ordered by: the score, or the
// x centre.  Role 0: keys 4t .. 4t+3, one float4 load; role 1: boxes 4t .. 4t+3, or with STRIDED boxes t + 1024 e, a wave's lanes then 16 bytes
// apart instead of 64.  flag: role 0, workgroup 0 "the scores came in sorted"; role 1 "every box of mine is plain" (tested on the box the key
// is made of, as sort_count_body does)
template <bool STRIDED>
__device__ __forceinline__ void sort_build_keys(const int role, const float* __restrict__ s, const float4* __restrict__ bx, const int n, const int N,
                                                const int r, const int mode3d, const float zlo, const float zscale, u64 (&k)[4], float (&val)[4],
                                                int& flag) {
    const int t = threadIdx.x;
    flag = 1;
    if (role == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = 0.0f;
        if (4 * t + 3 < N && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            const float4 q = reinterpret_cast<const float4*>(s)[t];
            val[0] = q.x; val[1] = q.y; val[2] = q.z; val[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (4 * t + e < n) val[e] = s[4 * t + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = (4 * t + e < n) ? (((u64)gnms_desc_key(val[e]) << 32) | (unsigned)(4 * t + e)) : ~0ull;   // (sort_key_of)
        if (r == 0) {                                                  // ascending keys in index order = the scores came in sorted
            const u64 next = (4 * t + 4 < n) ? sort_key_of(0, s, nullptr, 4 * t + 4, 0, 0.0f, 0.0f) : ~0ull;
            flag = (4 * t + 1 >= n || k[0] < k[1]) && (4 * t + 2 >= n || k[1] < k[2]) && (4 * t + 3 >= n || k[2] < k[3]) && (4 * t + 4 >= n || k[3] < next);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = STRIDED ? t + 1024 * e : 4 * t + e;
            k[e] = ~0ull;
            val[e] = 0.0f;
            if (i < n) {
                const float4 v = bx[i];
                k[e] = column_key(v, i, mode3d, zlo, zscale);
                val[e] = v.x + v.z;                                    // (column_key's x centre)
                flag &= box_orders_plainly(v) ? 1 : 0;
            }
        }
    }
}

// what only one workgroup per image and role does: the flags (it holds every key, so it decides alone; all: role 0 "came in sorted", role 1
// "every box is plain"), the counters, the call counter, the hand-off granules
__device__ __forceinline__ void sort_image_flags(const ImgPtrs& I, const int role, const bool has_boxes, const int all) {
    const int t = threadIdx.x;
    if (role == 0) {
        if (t < 8 && !(has_boxes && t == 6)) I.misc[t] = (t == 2) ? all : 0;               // ([6]: the x sort's)
        if (t == 8) I.misc[8] = gnms_next_epoch(I.misc[8]);
        for (int i = t; i < 17 * 32; i += 1024) I.gran[i] = 0ull;
    } else if (t == 0) {
        I.misc[6] = all ? 0 : 1;
    }
}

// key of input index idx has rank `rank`: what it leaves behind (sv, bv: its score and box, requested before the rank was known)
__device__ __forceinline__ void sort_store_ranked(const ImgPtrs& I, const int role, const int rank, const int idx, const float sv, const float4 bv,
                                                  const bool has_boxes, long long* __restrict__ order_img, const int mode3d) {
    if (role == 0) {
        I.order[rank] = idx;
        I.rankof[idx] = rank;
        I.sscore[rank] = sv;
        if (has_boxes) I.rbox[rank] = bv;                              // (the from-boxes layer: row boxes of the bit matrix)
        if (order_img) order_img[rank] = idx;
    } else {
        column_store(I, rank, idx, bv, mode3d);
    }
}
// padding ranks map to themselves (order is a permutation of [0, N)): workgroup r of 16 takes its share
__device__ __forceinline__ void sort_store_padding(const ImgPtrs& I, const int n, const int N, const int r, long long* __restrict__ order_img) {
    const int kp = n + r * 1024 + (int)threadIdx.x;
    if (kp < N) {
        I.order[kp] = kp; I.rankof[kp] = kp; I.sscore[kp] = 0.0f;
        if (order_img) order_img[kp] = kp;
    }
}

// The run sort and the ranks of workgroup r on the keys its threads hold: any split of the image's keys into 16 x 64 x 4 does.
// housekeep: workgroup 0 also decides the flags here (sort_hist_rank_body has done that before it falls back to this)
__device__ __forceinline__ void ranked_runs_finish(u64 (&k)[4], const int flag, const bool housekeep, SortTicks& T, const int path,
                                                   const float* __restrict__ s, const float4* __restrict__ bx, const int N, const int n,
                                                   const ImgPtrs& I, long long* __restrict__ order_img, const int r, const int b, const int role,
                                                   const int mode3d) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                          // [16][256]: the image as 16 sorted runs (padding ~0: behind everything)
    __shared__ int part[3][kRankRunKeys];                              // partial counts of quarters 1 .. 3
    const int t = threadIdx.x;
    wave_sort_256(k);
    T.tick();
#pragma unroll
    for (int e = 0; e < 4; ++e) keys[4 * t + e] = k[e];
    if (housekeep && r == 0) {
        const int all = __syncthreads_and(flag);                       // (also: the runs are in LDS)
        sort_image_flags(I, role, bx != nullptr, all);
    } else {
        __syncthreads();
    }
    T.tick();
    const int key = t & (kRankRunKeys - 1), quarter = t >> 8;
    const u64 mine = keys[r * kRankRunKeys + key];
    const bool live = mine != ~0ull;
    const int idx = (int)((unsigned)mine & (role == 0 ? 0xffffffffu : kColIdxMask));
    // what leaves with the key -- its score, its box -- is fetched by INPUT index, known before the searches: requested here (sort_merge_body)
    float sv = 0.0f;
    float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (quarter == 0 && live) {
        if (role == 0) sv = s[idx];
        if (bx) bv = bx[idx];
    }
    int cnt = 0;
    if (live) {
        const u64* q4 = keys + quarter * 4 * kRankRunKeys;             // the four runs of this quarter
        int pos[4] = {0, 0, 0, 0};
#pragma unroll
        for (int h = kRankRunKeys / 2; h >= 1; h >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) pos[j] += (q4[j * kRankRunKeys + pos[j] + h - 1] < mine) ? h : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt += (quarter * 4 + j == r) ? key : pos[j] + ((q4[j * kRankRunKeys + pos[j]] < mine) ? 1 : 0);
        if (quarter) part[quarter - 1][key] = cnt;
    }
    T.tick();
    __syncthreads();
    T.tick();
    if (quarter == 0 && live) sort_store_ranked(I, role, cnt + part[0][key] + part[1][key] + part[2][key], idx, sv, bv, bx != nullptr, order_img, mode3d);
    if (role == 0) sort_store_padding(I, n, N, r, order_img);
    T.tick();
    T.flush(I, b, r, role, path);
}

// (workgroup r of 16 of image b, role): grid (16, B, roles), 1024 threads, 4096 * 8 bytes of dynamic LDS; 2048 < N <= 4096
__device__ __forceinline__ void sort_ranked_runs_body(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                      const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                      long long* __restrict__ order_out, const int r, const int b, const int role,
                                                      const int mode3d = 0) {
    SortTicks T;
    T.tick();
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float* s = scores + (size_t)b * N;
    const float4* bx = boxes ? reinterpret_cast<const float4*>(boxes) + (size_t)b * N : nullptr;
    float zlo = 0.0f, zscale = 0.0f;
    if (role == 1 && mode3d > 1) block_z_bands(bx, n, mode3d, &zlo, &zscale);
    u64 k[4];
    float val[4];
    int flag;                                                          // workgroup 0: role 0 "the scores came in sorted", role 1 "every box is plain"
    sort_build_keys<false>(role, s, bx, n, N, r, mode3d, zlo, zscale, k, val, flag);
    T.tick();
    ranked_runs_finish(k, flag, true, T, 0, s, bx, N, n, I, order_out ? order_out + (size_t)b * N : nullptr, r, b, role, mode3d);
}

// ------------------------------------------------------------------------------------------------
// K1 for 2048 < N <= 4096 by HISTOGRAM (round 13): the same launch, grid and results as the ranked runs, without their sort.  There every one
// of the 16 workgroups of an image and role sorts all sixteen runs in registers -- 36 compare-exchange stages on four 64-bit keys per lane,
// 21 of them across lanes -- to rank one run.  A key's rank is the number of keys below it, and a histogram over a monotone function of the
// key (sort_bins.h) gives nearly all of that: workgroup (r, image, role)
//   builds every key of its image and role and reduces the finite minimum and maximum of the value they are ordered by (min / max do not
//     depend on the order: the 16 workgroups bin alike, as with block_z_bands);
//   bins each key, one LDS atomic per key on a histogram zeroed while the loads were in flight; the value the atomic returns is the key's
//     slot in its bin;
//   scans the bins (4 per thread, gnms_add_scan32 per wave, wave totals through LDS), the barrier of that scan deciding "some bin holds more
//     than `cap` keys" on the way, and scatters the keys into bin order in LDS (the order inside a bin is whatever the atomics made it);
//   ranks the bins that start in positions 256 r .. 256 r + 255 of that array: one thread per position counts the smaller keys of its key's
//     bin, rank = bin start + count.  Keys are distinct, so the rank is exact whatever the slot order was.
// Uniform scores and x centres put 2 keys into the average key's bin and at most 7-13 into any; values piled onto a few points (equal scores,
// a detector's scores near zero, one far outlier stretching the range) fill single bins, and past `cap` keys in one bin the workgroup goes
// on with the run sort on the keys it holds (ranked_runs_finish) -- for the whole image and role alike, the histogram being the same in all 16.
// The stores land nearly contiguously per workgroup (ranks 256 r .. of the image) instead of scattered over the image.
// ------------------------------------------------------------------------------------------------
constexpr int kHistBins = 4096;
constexpr int kHistCap = 96;             // keys in one bin past which the run sort takes over: the histogram still wins with 112 keys in EVERY bin, loses with 158 (LABNOTES R13.4)
constexpr int kHistCapMax = 1024 - kRankRunKeys + 1;   // (the bins a workgroup ranks fit its 1024 threads)
constexpr int kSortPathSlot = 10;        // misc[10 + role]: how the histogram sort went for this image and role, 1 = by histogram, 2 = fell back

__device__ __forceinline__ void sort_hist_rank_body(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                    const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                    long long* __restrict__ order_out, const int cap_arg, const int r, const int b, const int role,
                                                    const int mode3d = 0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                          // [4096] the image's keys in bin order
    const int cap = cap_arg < kHistCapMax ? cap_arg : kHistCapMax;
    __shared__ __attribute__((aligned(16))) unsigned hist[kHistBins];  // counts, then the bins' starts
    __shared__ unsigned short binof[kRankRuns * kRankRunKeys];         // bin of the key at a position
    __shared__ float red[2][16];
    __shared__ unsigned wtot[16];
    SortTicks T;
    T.tick();
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* s = scores + (size_t)b * N;
    const float4* bx = boxes ? reinterpret_cast<const float4*>(boxes) + (size_t)b * N : nullptr;
    long long* order_img = order_out ? order_out + (size_t)b * N : nullptr;
    reinterpret_cast<uint4*>(hist)[t] = make_uint4(0u, 0u, 0u, 0u);
    float zlo = 0.0f, zscale = 0.0f;
    if (role == 1 && mode3d > 1) block_z_bands(bx, n, mode3d, &zlo, &zscale);
    u64 k[4];
    float val[4];
    int flag;
    sort_build_keys<true>(role, s, bx, n, N, r, mode3d, zlo, zscale, k, val, flag);
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k[e] != ~0ull && fabsf(val[e]) < INFINITY) { lo = fminf(lo, val[e]); hi = fmaxf(hi, val[e]); }
    lo = gnms_wave_min_f(lo); hi = gnms_wave_max_f(hi);
    if (lane == 0) { red[0][wave] = lo; red[1][wave] = hi; }
    if (r == 0) {
        const int all = __syncthreads_and(flag);                       // (also: the histogram is zero, the waves' ranges are in LDS)
        sort_image_flags(I, role, bx != nullptr, all);
    } else {
        __syncthreads();
    }
    lo = gnms_wave_min_f(lane < 16 ? red[0][lane] : INFINITY);
    hi = gnms_wave_max_f(lane < 16 ? red[1][lane] : -INFINITY);
    const unsigned bpb = (unsigned)kHistBins / (unsigned)((role == 1 && mode3d > 1) ? mode3d : 1);   // bins per z band
    const float scale = hist_bin_scale(lo, hi, bpb);
    T.tick();
    unsigned bin[4], slot[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bin[e] = 0u; slot[e] = 0u;
        if (k[e] != ~0ull) {
            bin[e] = (role == 0) ? hist_bin_desc(val[e], lo, scale, bpb) : (unsigned)(k[e] >> 60) * bpb + hist_bin_asc(val[e], lo, scale, bpb);
            slot[e] = atomicAdd(&hist[bin[e]], 1u);
        }
    }
    __syncthreads();
    T.tick();
    const uint4 c = reinterpret_cast<const uint4*>(hist)[t];           // bins 4t .. 4t+3
    const unsigned sum = c.x + c.y + c.z + c.w;
    const unsigned inc = gnms_add_scan32(sum);
    if (lane == 63) wtot[wave] = inc;
    const unsigned most = max(max(c.x, c.y), max(c.z, c.w));
    const int over = __syncthreads_or(most > (unsigned)cap);           // (also: the waves' totals are in LDS)
    if (r == 0 && t == 0) I.misc[kSortPathSlot + role] = over ? 2 : 1;
    if (over) {
        ranked_runs_finish(k, flag, false, T, 2, s, bx, N, n, I, order_img, r, b, role, mode3d);
        return;
    }
    {
        const unsigned carry = (unsigned)__builtin_amdgcn_readlane((int)gnms_add_scan32((lane < wave) ? wtot[lane] : 0u), 63);
        const unsigned ex = carry + inc - sum;
        reinterpret_cast<uint4*>(hist)[t] = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
    }
    __syncthreads();
    T.tick();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (k[e] != ~0ull) {
            const unsigned p = hist[bin[e]] + slot[e];                 // (< n: the bins' counts add up to n)
            keys[p] = k[e];
            binof[p] = (unsigned short)bin[e];
        }
    }
    __syncthreads();
    T.tick();
    // Workgroup r ranks the bins that START in positions 256 r .. 256 r + 255 -- whole bins, not the positions themselves: which key of a bin
    // stands at which of its positions is the atomics' order and differs from workgroup to workgroup, what is IN a bin does not.  Those bins
    // end before position 256 r + 255 + cap, so thread t takes position 256 r + t and the first 255 + cap threads cover them (cap <= kHistCapMax).
    const int p = r * kRankRunKeys + t;
    bool ranked = false;
    int idx = 0, rank = 0;
    float sv = 0.0f;
    float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p < n && t < kRankRunKeys + cap - 1) {
        const int mb = binof[p];
        const int start = (int)hist[mb];
        if (start >= r * kRankRunKeys && start < (r + 1) * kRankRunKeys) {
            ranked = true;
            const int end = (mb + 1 < kHistBins) ? (int)hist[mb + 1] : n;
            const u64 mine = keys[p];
            idx = (int)((unsigned)mine & (role == 0 ? 0xffffffffu : kColIdxMask));
            if (role == 0) sv = s[idx];                                // (fetched by input index, under the count: sort_merge_body)
            if (bx) bv = bx[idx];
            rank = start;
            for (int j = start; j < end; ++j) rank += (keys[j] < mine) ? 1 : 0;
        }
    }
    T.tick();
    if (ranked) sort_store_ranked(I, role, rank, idx, sv, bv, bx != nullptr, order_img, mode3d);
    if (role == 0) sort_store_padding(I, n, N, r, order_img);
    T.tick();
    T.flush(I, b, r, role, 1);
}

// ------------------------------------------------------------------------------------------------
// K1 for N <= 2048 (round 5): the same two sorts by COUNTING, spread over the machine.  Up to 1024 keys one workgroup per (image, role)
// sorted them in LDS: 4-5 us of merge passes on one CU inside a 9-12-us launch that left 240 CUs idle -- the longest launch in front of the
// chain at the reference's own sizes.  A key's position in the sorted order is the number of keys below it (keys are distinct: the index is
// in the low bits), and that needs no sort at all: workgroup (block, image, role) takes 64 keys, every workgroup holds ALL keys of its
// image in LDS, thread (key, segment) counts the keys of one sixteenth of the image below its own, an LDS atomic adds the sixteen counts,
// and the 64 results leave exactly as the merge kernel's do.  N / 64 workgroups per image and role: 256 at B = 8, N = 1024.
// ------------------------------------------------------------------------------------------------
// FUSED (round 6, one_launch_kernel; strong_gran and the slot numbers: gnms_device.h): the same workgroup as a ROLE of the one launch of a small image.  Nothing of the workspace is
// zeroed or counted here (the launch's tag comes from its caller and the flags are strong granules, see there); everything another
// workgroup of the launch reads leaves through agent-scope stores, and the workgroup's last act is its "sorted" flag.
template <int KPW, bool FUSED = false>   // keys per workgroup: 64, or 32 where that still is one round of the machine (B = 1, N = 4096: 10.5 -> ? us)
__device__ __forceinline__ void sort_count_body(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                long long* __restrict__ order_out, int mode3d, const int blk, const int b, const int role,
                                                const unsigned tag = 0u) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                          // [NP] all keys of the image (padding ~0: behind everything)
    __shared__ int rk[64];
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int t = threadIdx.x, lane = t & (KPW - 1), seg = t / KPW;
    const int NP = (N + 63) & ~63;
    const float* s = scores + (size_t)b * N;
    const float* bx = boxes ? boxes + (size_t)b * N * 4 : nullptr;
    float zlo = 0.0f, zscale = 0.0f;
    if (role == 1 && mode3d > 1) block_z_bands(reinterpret_cast<const float4*>(bx), n, mode3d, &zlo, &zscale);
    const int k = blk * KPW + lane;                                    // (k < NP)
    // key k is input index k: what leaves with it -- its score, its box -- needs no index from the sorted keys and is requested here, in front
    // of everything (round 6: fetched by `idx` behind the count it was one more exposed memory round trip at the end of every workgroup)
    float pre_s = 0.0f;
    float4 pre_b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (seg == 0 && k < n) {
        if (role == 0) pre_s = s[k];
        if (bx) pre_b = reinterpret_cast<const float4*>(bx)[k];
    }
    int flag = 1;                                                      // role 1: "every box is plain" (workgroup 0 decides, below)
    if (role == 0) {
        for (int i = t; i < NP; i += 1024) keys[i] = (i < n) ? sort_key_of(0, s, bx, i, mode3d, zlo, zscale) : ~0ull;
    } else {
        // (the plain test on the box the key is made of: as a pass of its own over the boxes it was a second memory round trip of workgroup 0,
        // the one every launch of this kernel ends with)
        for (int i = t; i < NP; i += 1024) {
            u64 key = ~0ull;
            if (i < n) {
                const float4 v = reinterpret_cast<const float4*>(bx)[i];
                key = column_key(v, i, mode3d, zlo, zscale);
                flag &= box_orders_plainly(v) ? 1 : 0;
            }
            keys[i] = key;
        }
    }
    if (t < 64) rk[t] = 0;
    __syncthreads();
    const u64 mine = keys[k];
    {
        const int per = NP / (1024 / KPW);                             // a multiple of 4 (KPW = 32: the launcher asks for NP % 128 == 0)
        const u64* p = keys + seg * per;
        int c = 0;
        for (int j = 0; j < per; j += 4) c += (p[j] < mine ? 1 : 0) + (p[j + 1] < mine ? 1 : 0) + (p[j + 2] < mine ? 1 : 0) + (p[j + 3] < mine ? 1 : 0);
        if (c) atomicAdd(&rk[lane], c);
    }
    // what only one workgroup per image and role does: the "already sorted" / "every box is plain" flags (every workgroup holds every key,
    // so the first one decides alone), the counters, the call counter, the hand-off granules
    if (blk == 0 && role == 0) {
        for (int i = t; i + 1 < n; i += 1024) flag &= keys[i] < keys[i + 1];          // ascending keys in index order = the scores came in sorted
    }
    const int all = __syncthreads_and(flag);                           // (also: every count has landed in rk)
    if (blk == 0) {
        if (role == 0) {
            if constexpr (FUSED) {
                if (t < 8 && !(boxes && t == 6)) coh_store(I.misc + t, (t == 2) ? all : 0);
            } else {
                if (t < 8 && !(boxes && t == 6)) I.misc[t] = (t == 2) ? all : 0;           // ([6]: the x sort's)
                if (t == 8) I.misc[8] = gnms_next_epoch(I.misc[8]);
                for (int i = t; i < 17 * 32; i += 1024) I.gran[i] = 0ull;
            }
        } else if (t == 0) {
            if constexpr (FUSED) coh_store(I.misc + 6, all ? 0 : 1); else I.misc[6] = all ? 0 : 1;
        }
    }
    if (seg == 0) {
        if (k < n) {
            const int rank = rk[lane];
            const int idx = (int)((unsigned)mine & (role == 0 ? 0xffffffffu : kColIdxMask));
            if (role == 0) {
                if constexpr (FUSED) {
                    coh_store(I.order + rank, idx);
                    coh_store(I.rankof + idx, rank);
                    coh_store(I.sscore + rank, pre_s);
                    if (boxes) coh_store_f4(I.rbox + rank, pre_b);
                } else {
                    I.order[rank] = idx;
                    I.rankof[idx] = rank;
                    I.sscore[rank] = pre_s;
                    if (boxes) I.rbox[rank] = pre_b;
                }
                if (order_out) order_out[(size_t)b * N + rank] = idx;
            } else {
                if constexpr (FUSED) {
                    coh_store(I.xidx + rank, idx);
                    coh_store_f4(I.xbox + rank, pre_b);
                } else {
                    column_store(I, rank, idx, pre_b, mode3d);
                }
            }
        } else if (k < N && role == 0) {                               // padding ranks map to themselves (order is a permutation of [0, N))
            if constexpr (FUSED) { coh_store(I.order + k, k); coh_store(I.rankof + k, k); coh_store(I.sscore + k, 0.0f); }
            else { I.order[k] = k; I.rankof[k] = k; I.sscore[k] = 0.0f; }
            if (order_out) order_out[(size_t)b * N + k] = k;
        }
    }
    if constexpr (FUSED) {
        __builtin_amdgcn_s_waitcnt(0x0f70);                            // vmcnt(0): this wave's stores are acknowledged ...
        __syncthreads();                                               // ... every wave's are
        if (t == 0) coh_store(I.gran + (size_t)(1 + role) * 32 + blk, strong_gran(tag, kSlotSort + 32u * (unsigned)role + (unsigned)blk));
    }
}

template <int KPW>
__global__ __launch_bounds__(1024) void sort_count_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                          const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                          long long* __restrict__ order_out, int mode3d) {
    sort_count_body<KPW>(scores, boxes, N, counts, ws, L, order_out, mode3d, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

}  // namespace
}  // namespace gnms
