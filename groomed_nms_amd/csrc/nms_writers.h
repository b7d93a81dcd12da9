// nms_writers.h -- the matrix writers as ROLES of a launch: device functions only, no kernel.  Their kernels: tail_write_kernel
// (nms_tail_write_launch.h), iou2d_self_kernel and one_launch_boxes_kernel (nms_layer.hip).
#pragma once
#include "iou_tile.h"
#include "iou3d_tile.h"
#include "iou3d_sym.h"

namespace {   // internal linkage: the header is included by several translation units

using namespace gnms;

// ------------------------------------------------------------------------------------------------
// The matrix write as a ROLE inside the launch of the per-image chain (masked from-boxes layer, gnms_forward_with_iou2d).
// Nothing in that layer reads the matrix, so the write is independent of the chain sorts -> threshold bits -> K3..K6.  As launches of
// their own the chain K3..K6 (one workgroup per image: 8 of 256 CUs at B = 8) ran strictly behind the write; as two streams the fork
// and join cost more than the overlap bought (LABNOTES.md 3.2d).  tail_write_kernel is both in ONE launch: the first B x nsb workgroups ARE
// the chain (the device functions of tail_kernel), the others write the matrix.  The launch asks for the chain's LDS (> 80 KiB), so a
// CU holds ONE workgroup: the chain workgroups are dispatched first and have a CU each to themselves (beside the write they run
// within 10 % of their stand-alone time; sharing a CU with streaming waves they ran 1.5-3x slower), the other CUs stream the matrix;
// when a chain workgroup retires, a writer still waiting in the grid takes its CU.
// A chunk = 16 wave tiles of tile_rows x 256 entries (tile_rows full rows of one image at N = 4096), written by the 16 waves of a
// workgroup with iou2d_tile -- the tile code of gnms_iou2d, so the matrix is the same bit for bit.
// Measured and dropped: slices of the write ALSO inside the sort launches and the bit-matrix launch (7 % / 5 % / 10-20 % of the rows,
// behind those kernels' own workgroups in the grid).  The sort and bit-matrix workgroups then share their CUs with streaming waves
// and slow down by more than the slices save: sort runs 7.8 -> 15.6 us, merges 5.9 -> 15.0, bit matrix 24 -> 46, chain + rest of the
// write 114 -> 98 (B = 8, N = 4096: 0.172 -> 0.173-0.184 ms per step for every split tried).
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int write_chunk_count(int N, int nimg, int tile_rows, int row0, int row_end) {
    if (row_end <= row0) return 0;
    const long tiles = (long)nimg * ((N + gnms_iou::kWaveCols - 1) / gnms_iou::kWaveCols) * ((row_end - row0 + tile_rows - 1) / tile_rows);
    return (int)((tiles + 15) >> 4);
}

// what the writers compute: SRC = kFromBoxes: `in` = boxes [B][N][4], lib/core.py iou (iou2d_tile);
// SRC = kFromRecords: `in` = corner-AABB records [B][N][12], 0.5 * (1 + GIoU3D) with the guard band around `thr` (nms_overlap3d_tile)
template <bool VEC, int SRC>
__device__ __forceinline__ void write_chunk(const float* __restrict__ in, int N, float* __restrict__ out, long ld, int nimg, int tile_rows,
                                            int row0, int row_end, float thr, int chunk) {
    using namespace gnms_iou;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncc = (N + kWaveCols - 1) / kWaveCols;
    const int nrt = (row_end - row0 + tile_rows - 1) / tile_rows;
    const int per_img = ncc * nrt;
    const int t = chunk * 16 + wave;                               // tiles numbered image-major, column chunk fastest
    if (t >= per_img * nimg) return;
    const int img = t / per_img;
    const int r = t - img * per_img;
    const int rt = r / ncc, cc = r - rt * ncc;
    if (SRC == kFromRecords)
        gnms_iou3d::nms_overlap3d_tile<VEC>(in, in, N, N, out, ld, img, row0 + rt * tile_rows, cc * kWaveCols, lane, tile_rows, row_end, thr);
    else
        iou2d_tile<VEC>(in, in, N, N, out, ld, img, row0 + rt * tile_rows, cc * kWaveCols, lane, tile_rows, row_end);
}

// PERSISTENT writers: one workgroup stays on its CU and claims chunk after chunk from `counter` (zeroed by the sort kernels of this
// call), one claim ahead so that the atomic's round trip hides behind the chunk in progress.  Claims are the ONLY cross-workgroup
// traffic of the launch: anything that needs a release/acquire fence between workgroups (the whole chain sorts -> bits -> K3..K6 as
// tasks of one persistent launch was the plan) is out of the question beside the write stream -- one __threadfence() per chunk
// (buffer_wbl2 + buffer_inv at agent scope) took this launch from 0.115 to 1.13 ms.  (Ordinary workgroups of one chunk each
// leave the CU empty between a workgroup's last wave and the next workgroup's start, and with one workgroup per CU nothing covers
// that gap: 116 against 107 us.  One claim per WAVE tile serialises on the counter: 16384 device-scope atomics on one address took
// 430 us.)
template <bool VEC, int SRC>
__device__ __forceinline__ void writers_persistent(const float* __restrict__ in, int N, float* __restrict__ out, long ld, int nimg,
                                                   int tile_rows, int row0, int row_end, float thr, int* counter) {
    __shared__ int s_next[2];
    const int nchunks = write_chunk_count(N, nimg, tile_rows, row0, row_end);
    if (threadIdx.x == 0) s_next[0] = atomicAdd(counter, 1);
    __syncthreads();
    int cur = s_next[0], ph = 0;
    while (cur < nchunks) {
        int nx = 0;
        if (threadIdx.x == 0) nx = atomicAdd(counter, 1);          // the claim after this one, in flight during the chunk
        write_chunk<VEC, SRC>(in, N, out, ld, nimg, tile_rows, row0, row_end, thr, cur);
        if (threadIdx.x == 0) s_next[ph ^ 1] = nx;
        __syncthreads();
        ph ^= 1;
        cur = s_next[ph];
    }
}

// STAGED writers (2D, N <= 4096): what keeps the persistent writers above from the rate of a plain store stream is vmcnt.  On gfx9
// loads, stores and returning atomics retire through ONE in-order counter, so the wave that waits for its next tile's boxes (5 loads)
// first waits for the 16 stores of the tile before, and thread 0, waiting for its claim, drains wave 0's stores while 15 waves sit at
// the barrier -- at 16 waves per CU nothing covers those gaps (tail_write_kernel 0.115 ms where gnms_iou2d's many small workgroups
// take 0.100).  Here the steady state has no vector load at all:
//   * the image's boxes are staged in LDS once per (workgroup, image) -- the chain's dynamic LDS, unused by writer workgroups -- and a
//     tile reads its column and row boxes from there (lgkmcnt);
//   * every image has its own claim counter (misc[5] of its workspace, zeroed by its sort) and a workgroup starts on image
//     (index mod B), moving on when that image is exhausted: 1-2 stagings per workgroup instead of B;
//   * the claim for the unit after next is issued BEFORE the tile's stores and consumed after them, the rows unrolled so that the
//     compiler counts the stores behind it and waits with vmcnt(8), not vmcnt(0).  (The atomic's address is made lane-dependent on
//     purpose: with a wave-uniform address the compiler's atomic optimizer wraps it in a readfirstlane that needs the result at once.)
// A unit = 16 wave tiles of 8 rows x 256 columns, numbered row band major inside an image.  (Rows per tile, B = 8: 16 -> 8 took the
// launch at N = 4096 from 102.5 to 93.0 us and the large-image launch at N = 16384 from 1.57 to 1.45 ms -- twice as many, shorter units
// even out what 2048 units on 248 workgroups leave uneven; 4 rows lose again, 111 us / 1.77 ms.)
constexpr int kStagedRows = 8;

// claim0 / claim_stride: image i's claim counter is claim0[i * claim_stride] (the layer: misc[5] of the image's workspace; gnms_iou2d:
// a zeroed array of its own); first_wg: blockIdx.x of the first writer workgroup of the launch
template <bool VEC>
__device__ __forceinline__ void writers_staged_2d(const float* __restrict__ boxes, int N, float* __restrict__ out, long ld, int nimg, int* claim0,
                                                  size_t claim_stride, const int first_wg) {
    using namespace gnms_iou;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sbox = reinterpret_cast<float4*>(smem);                  // [N] boxes of the staged image
    __shared__ int s_claim[2];                                       // (image << 16 | unit) or -1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncc = (N + kWaveCols - 1) / kWaveCols;
    const int nrt = (N + kStagedRows - 1) / kStagedRows;
    const int units = (ncc * nrt + 15) >> 4;
    // thread 0 only: the image it claims from and how many images it has not yet seen exhausted
    int cur_img = ((int)blockIdx.x - first_wg) % nimg, left = nimg;
    // never 1 at run time, but not provably 0 either: keeps the claim's address lane-dependent in the compiler's eyes
    const int lane_dep = (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) >> 6);
    auto counter = [&](int img) { return claim0 + (size_t)img * claim_stride + lane_dep; };
    auto claim_now = [&]() -> int {                                  // the next unit of cur_img, or of the next image that has one
        while (left > 0) {
            const int u = atomicAdd(counter(cur_img), 1);
            if (u < units) return (cur_img << 16) | u;
            cur_img = cur_img + 1 == nimg ? 0 : cur_img + 1;
            --left;
        }
        return -1;
    };
    if (tid == 0) s_claim[0] = claim_now();
    __syncthreads();
    int cur = s_claim[0], ph = 0, staged = -1;
    // PLAIN images (every box divides plainly, iou_tile.h -- pixel boxes always do; decided once per staging): the tile runs
    // iou2d_rows_plain, and the lane's column boxes stay in registers from unit to unit while the wave keeps its column chunk (at
    // N = 4096 always: a unit is one band of 16 chunks) -- gathering them, their areas and the plain test were 17 % of a tile's VALU work.
    bool img_plain = false;
    int cols_of = -1;                                                // the column chunk `cp` holds (of the staged image)
    ColPairs cp;
    const bool fast_ok = VEC && (N & 3) == 0 && (N % kStagedRows) == 0;
    while (cur >= 0) {
        const int img = cur >> 16, u = cur & 0xffff;
        if (img != staged) {                                         // (every wave finished reading the old image before the last barrier)
            const float4* b4 = reinterpret_cast<const float4*>(boxes) + (size_t)img * N;
            bool ok = true;
            for (int i = tid; i < N; i += 1024) { const float4 v = b4[i]; sbox[i] = v; ok = ok && box_divides_plainly(v); }
            staged = img;
            cols_of = -1;
            img_plain = __syncthreads_and(ok) != 0;
        }
        int pre = 0;
        const bool claims = tid == 0 && left > 0;
        const int t = u * 16 + wave;                                 // (wave 0's tile always exists: it carries the claim)
        if (t < ncc * nrt) {
            const int rt = t / ncc, cc = t - rt * ncc;
            const int c0 = cc * kWaveCols;
            if (fast_ok && img_plain && c0 + 4 * kStagedRows <= N) { // (the first kStagedRows lanes hold the rows AND must own columns)
                if (cc != cols_of) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) colpairs_set(cp, j, sbox[min(c0 + 4 * lane + j, N - 1)]);
                    cols_of = cc;
                }
                const float4 ra = sbox[rt * kStagedRows + (lane & (kStagedRows - 1))];
                if (c0 + 4 * lane < N) {
                    if (claims) pre = atomicAdd(counter(cur_img), 1);                // in flight ahead of this tile's stores
                    float* o0 = out + (size_t)img * N * ld + (size_t)(rt * kStagedRows) * ld + c0 + 4 * lane;
                    iou2d_rows_plain<kStagedRows>(cp, ra, o0, ld);
                    asm volatile("" :: "v"(pre));                                    // every path waits for it here: vmcnt(8) on a full tile
                }
            } else {
                iou2d_tile_staged<VEC, kStagedRows>(sbox, 0, sbox + rt * kStagedRows, N, N, out + (size_t)img * N * ld, ld, rt * kStagedRows, c0, lane,
                    [&] { if (claims) pre = atomicAdd(counter(cur_img), 1); },
                    [&] { asm volatile("" :: "v"(pre)); });
            }
        }
        if (tid == 0) {
            int nx = -1;
            if (left > 0) {
                if (pre < units) nx = (cur_img << 16) | pre;
                else { cur_img = cur_img + 1 == nimg ? 0 : cur_img + 1; --left; nx = claim_now(); }
            }
            s_claim[ph ^ 1] = nx;
        }
        __syncthreads();
        ph ^= 1;
        cur = s_claim[ph];
    }
}

// SYMMETRIC writers (3D, round 3): the write role of tail_write_kernel for the cuboid overlap -- every unordered pair evaluated once
// (iou3d_sym.h), the all-pairs 3D writers being VALU-bound at the one workgroup per CU this launch runs at (3.2e).  A persistent
// 16-wave workgroup claims 128 x 128 macro tiles (upper triangle of every image, image-major) one claim ahead and alternates between
// TWO LDS tiles, so that ONE barrier per macro tile suffices: it publishes the tile for the mirrored pass AND the next claim, and the
// waves that finish their mirrored stores early already compute the next tile into the other buffer.
template <bool NT>
__device__ __forceinline__ void writers_sym_persistent(const float* __restrict__ rec, int N, float* __restrict__ out, long ld, int nimg, float thr,
                                                       int* counter) {
    using namespace gnms_iou3d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const tile0 = reinterpret_cast<float*>(smem);           // two LDS macro tiles, kSymTileBytes apart
    __shared__ int s_next[2];
    const int nt = (N + kSymT - 1) / kSymT;
    const int tpi = sym_tiles_per_image(N), total = tpi * nimg;
    if (threadIdx.x == 0) s_next[0] = atomicAdd(counter, 1);
    __syncthreads();
    int cur = s_next[0], ph = 0;
    while (cur < total) {
        int nx = 0;
        if (threadIdx.x == 0) nx = atomicAdd(counter, 1);          // the claim after this one, in flight during the tile
        const int img = cur / tpi;
        int I, J;
        sym_tile_of(cur - img * tpi, nt, &I, &J);
        const float* r = rec + (size_t)img * N * kRec;
        float* o = out + (size_t)img * N * ld;
        float* const tile = tile0 + (size_t)ph * (kSymTileBytes / sizeof(float));
        sym_tile_compute<16, NT>(r, N, o, ld, I, J, thr, tile);
        if (threadIdx.x == 0) s_next[ph ^ 1] = nx;
        __syncthreads();                                            // the tile is in LDS, the next claim is known; buffer ph ^ 1 is free
        if (I != J) sym_tile_mirror<16, NT>(N, o, ld, I, J, tile);
        ph ^= 1;
        cur = s_next[ph];
    }
}

}  // namespace
