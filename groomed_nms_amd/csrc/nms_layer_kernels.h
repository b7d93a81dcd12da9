// nms_layer_kernels.h -- the layer's non-template __global__ functions: the K1 wrappers, K2 for small images, K2s, K2c on the triangular
// tile set and K3.  nms_layer.hip launches every one of them and is the only unit of the library that includes this header; the templates
// and bodies they are made of (nms_kernels.h) are shared with the tail units, which launch none of these.
#pragma once
#include "nms_kernels.h"
#include "nms_leaders_kernel.h"

namespace gnms {
namespace {

// K1's non-template kernels (bodies and their description: nms_sort_kernels.h)
__global__ __launch_bounds__(1024) void sort_runs_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                         const int* __restrict__ counts, char* ws, gnms_ws_layout L, int P, int mode3d) {
    sort_runs_body(scores, boxes, N, counts, ws, L, P, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, mode3d);
}

__global__ __launch_bounds__(1024) void sort_ranked_runs_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                                const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                                long long* __restrict__ order_out, int mode3d) {
    sort_ranked_runs_body(scores, boxes, N, counts, ws, L, order_out, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, mode3d);
}

__global__ __launch_bounds__(1024) void sort_hist_rank_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                              const int* __restrict__ counts, char* ws, gnms_ws_layout L,
                                                              long long* __restrict__ order_out, int mode3d, int cap) {
    sort_hist_rank_body(scores, boxes, N, counts, ws, L, order_out, cap, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, mode3d);
}

// K2 for few, small images (round 5): bitmask_kernel (nms_kernels.h) gives a wave 64 rows x 256 columns, eight batches of eight 1-KiB loads one after the
// other -- at N = 500, B = 1 that is 16 busy waves on the whole machine and eight memory latencies in a row (8.8 us for 1 MB).  Here the 64
// rows of a rank block are dealt to the eight waves of a workgroup, eight rows each: ONE batch of loads per wave.  A wave's eight rows
// are eight consecutive bits = one BYTE of the column's word, so the partial results meet in LDS as the bytes of the words (byte stores),
// and four of the waves scatter the finished words.  Stores exactly the words bitmask_kernel<true> stores.  Needs ld % 4 == 0 and a
// 16-byte aligned matrix (VEC).
__global__ __launch_bounds__(512) void bitmask_small_kernel(const float* __restrict__ iou, int N, long ld, const int* __restrict__ counts,
                                                            float thr, char* ws, gnms_ws_layout L, int full) {
    __shared__ u64 words[256];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int kb = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    const int k0 = kb * 64;
    if (k0 >= n) return;
    const int c0 = (int)((blockIdx.x + kb) % gridDim.x) * 256;           // (rotated like bitmask_kernel's chunks)
    ImgPtrs I = img_ptrs(ws, L, b);
    const bool ident = I.misc[2] != 0;
    if (c0 >= n || (ident && c0 >= k0 + 64)) return;                     // (workgroup-uniform)
    const float* m = iou + (size_t)b * N * ld;
    const int myrank = k0 + lane;
    const int myrow = (myrank < n) ? I.order[myrank] : I.order[k0];
    const int nrows = min(64, n - k0);
    const u64 rowmask = (nrows >= 64) ? ~0ull : ((1ull << nrows) - 1ull);
    // the scatterers' ranks, asked for before the rows so that the two latencies overlap
    const int mycol = c0 + (int)threadIdx.x;
    int rk = mycol;
    if (threadIdx.x < 256 && mycol < n && !ident) rk = I.rankof[mycol];
    const int col0 = c0 + 4 * lane;
    const bool active = col0 + 3 < ld;
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int row = __builtin_amdgcn_readlane(myrow, wave * 8 + u);
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) v[u] = load_nt_f4(m + (size_t)row * ld + col0);
    }
    unsigned by[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const unsigned bit = 1u << u;
        by[0] |= !(v[u].x <= thr) ? bit : 0u;                            // lib/groomed_nms.py:250 (NaN -> removed)
        by[1] |= !(v[u].y <= thr) ? bit : 0u;
        by[2] |= !(v[u].z <= thr) ? bit : 0u;
        by[3] |= !(v[u].w <= thr) ? bit : 0u;
    }
    unsigned char* bytes = reinterpret_cast<unsigned char*>(words);
#pragma unroll
    for (int j = 0; j < 4; ++j) bytes[(4 * lane + j) * 8 + wave] = (unsigned char)by[j];
    __syncthreads();
    if (threadIdx.x < 256 && mycol < n && (full || rk < k0 + 64)) (I.W + (size_t)kb * L.NC)[rk] = words[threadIdx.x] & rowmask;
}

// K2s as a launch of its own (the check and its description: wsym_pair_bad, nms_kernels.h)
// (four pairs per wave, eight loads in flight, measured slower in round 3: 13.0 against 10.7 us at B = 8, N = 4096)
__global__ __launch_bounds__(256) void wsym_check_kernel(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int nb = (n + 63) >> 6;
    const int pairs = nb * (nb + 1) / 2;
    const int pr0 = blockIdx.x * 4 + (threadIdx.x >> 6);                         // pair index, row-major over kb <= jb
    if (pr0 >= pairs) return;
    if (I.misc[2] != 0) { if (pr0 == 0 && lane == 0) I.misc[3] = 1; return; }   // pre-sorted scores: W holds the triangle only
    const bool bad = wsym_pair_bad(I, L, n, nb, pr0, lane);
    if (__any(bad) && lane == 0) I.misc[3] = 1;                          // (every writer stores 1; the sort zeroed it)
}

// K2c on the triangular tile set (its description, tri_tile and tri_tile_count: nms_kernels.h)
__global__ __launch_bounds__(256) void bitmask_rec3d_kernel(int N, const int* __restrict__ counts, float thr, char* ws, gnms_ws_layout L) {
    using namespace gnms_iou3d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int n = gnms_count(counts, b, N);
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tri_tile_count(L.NB)) return;
    int kb, chunk;
    tri_tile(tile, &kb, &chunk);
    const int k0 = kb * 64, c0 = chunk * 256;
    if (k0 >= n || c0 >= n) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    Cols2 cols[2];
    int col[4];
    unsigned colbad = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        col[j] = c0 + 4 * lane + j;
        const float4* p = reinterpret_cast<const float4*>(I.rec + (size_t)I.order[col[j] < n ? col[j] : n - 1] * kRec);
        const float4 e = p[2];
        cols2_set(cols[j >> 1], j & 1, p[0], p[1], e);
        colbad |= (e.w != 0.0f) ? (1u << j) : 0u;
    }
    const float4* rp = reinterpret_cast<const float4*>(I.rec + (size_t)I.order[min(k0 + lane, n - 1)] * kRec);
    const float4 ru = rp[0], rv = rp[1], re = rp[2];
    const int nrows = min(64, n - k0);
    const bool cols_sane = __all(colbad == 0u);
    unsigned wd[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int rend = min(32, nrows - half * 32);
        for (int rr = 0; rr < rend; ++rr) {
            const int r = half * 32 + rr;
            auto bc = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); };
            Row a;
            a.vol = bc(ru.x); a.y0 = bc(ru.y); a.y1 = bc(ru.z); a.x0 = bc(ru.w); a.x1 = bc(rv.x); a.z0 = bc(rv.y); a.z1 = bc(rv.z);
            a.lx = bc(re.x); a.ly = bc(re.y); a.lz = bc(re.z); a.bad = bc(re.w);
            const unsigned bit = 1u << rr;
            float q[4];
            nms_overlap3d_guarded4(a, cols, colbad, cols_sane, thr, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) wd[half][j] |= !(q[j] <= thr) ? bit : 0u;
        }
    }
    u64* Wk = I.W + (size_t)kb * L.NC;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (col[j] < n) Wk[col[j]] = ((u64)wd[1][j] << 32) | wd[0][j];
}

}  // namespace
}  // namespace gnms
