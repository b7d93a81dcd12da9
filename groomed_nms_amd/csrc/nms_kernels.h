// nms_kernels.h -- GrooMeD-NMS forward kernels for gfx950 (MI355X): sort, threshold bit-matrix, greedy
// leader scan, group attribution, grouping + default (masked) rescoring, validity split.
//
// Reference: lib/groomed_nms.py:10-129 differentiable_nms and :208-270 get_groups.
//
// Formulation (see DESIGN.md for the derivation).  get_groups repeatedly takes the highest-scoring
// remaining box as leader L and removes every remaining box i with NOT(iou[i][L] <= thr) (:249-262);
// the ones with iou[i][L] > thr, capped at group_size+1 in score order, form the group (:253-255).
// That is classical greedy NMS plus "each box remembers the first leader that removed it".  We
// therefore never materialise the score-sorted copy of the matrix (:48) nor the N x N inversion
// matrix (:65,:108):
//   K1 sort_scores   stable descending argsort per image                       (one workgroup / image, LDS bitonic)
//   K2 bitmask       the ONE full read of the N x N fp32 matrix -> N*N/8-byte bit matrix W
//                    (HBM-bound: 4 N^2 bytes in, N^2/8 out)                      <- dominant kernel
//   K3 leaders       sequential scan over 64-rank blocks on the bit matrix       (one workgroup / image)
//   K4 attribute     first-remover per box, parallel over rank blocks
//   K5 groups        membership (strict >), cap, head, CSR of groups; default rescoring fused
//   K6 finalize      clamp / threshold / second sort / valid + invalid lists / output order
//
// This is the LAYER's header: the templates and bodies of K2, K2s, K4..K6 and the tails.  Its includers are the layer's units: nms_layer.hip
// (through nms_layer_kernels.h / nms_backward_kernels.h / nms_solve_kernels.h / nms_one_launch.h), the nms_tail_*.hip units (nms_tail_launch.h)
// and the nms_tail_write_*.hip units (nms_tail_write_launch.h).  What the rest of the library borrows is in the three headers below:
// gnms_device.h (device primitives, no kernel), nms_sort_kernels.h (K1) and nms_scan_kernels.h (K3).  A header that more than one .hip file
// includes defines no non-template __global__ function that one of its includers does not launch (the build treats an unused one as an
// error): the layer's non-template kernels are in nms_layer_kernels.h, which nms_layer.hip alone includes.
#pragma once
#include <type_traits>
#include "gnms_device.h"
#include "nms_sort_kernels.h"
#include "nms_scan_kernels.h"
#include "iou_tile.h"

namespace gnms {
namespace {   // internal linkage: the header is included by several translation units

// ------------------------------------------------------------------------------------------------
// K2: threshold bit matrix -- the ONE full read of the N x N fp32 matrix (HBM-read bound).
// One wave = 64 rank-rows x 256 input columns.  Rows order[64*kb + r] are contiguous 4N-byte streams
// whatever the permutation, so the row gather is free; lane t accumulates, for each of its 4 columns c,
//     word(c) = sum_r  !(iou[order[64 kb + r]][c] <= thr) << r
// i.e. column c of the thresholded matrix with its bits already in RANK order, and scatters it to
// W[kb][rankof[c]] so that every later kernel reads W contiguously (rank x rank space).
// Tuning (tools/bw_variants.hip, MI355X): ROLLED row loops with 8 x 1-KiB non-temporal loads in flight per
// wave keep the kernel at 63 VGPRs = 8 waves/SIMD; that beats the fully unrolled 64-load version
// (256 VGPRs, 1 wave/SIMD) by 18 % and reaches 5.6 TB/s with the scatter (6.0 TB/s without).
// ------------------------------------------------------------------------------------------------
constexpr int kMaskWaves = 8;       // waves per workgroup: 8 x 256 = 2048 columns
constexpr int kMaskRB = 8;          // rows (1-KiB loads) in flight per wave

// Rows of W out of an LDS row buffer, WRITE-THROUGH (round 9): `words` words (a row of NC, or KBW adjacent rows: they are adjacent in W as
// in LDS) from `src` to `dst`, every lane 16 bytes per pass -- ds_read_b128, one 16-byte buffer store with sc1 (aux = 16).  A plain store
// leaves its line dirty in the XCD's L2, and the end-of-kernel release writes all of them back while the next launch waits: 16.8 MB of W at
// B = 8, N = 4096, 1.5 us at the end of this kernel and 0.8 at the start of tail_write_kernel (LABNOTES R9.1).  An sc1 store leaves as it is issued, while other workgroups still
// compute.  (8-byte sc1 stores cost 2.7x the time per byte: the pairs matter.)  Needs words % 2 == 0 and 16-byte aligned src / dst:
// NC = round_up(N, 4), the rows of W start 32-byte aligned, the row buffer is the 16-byte aligned base of the LDS.  Every consumer of W runs
// in a later launch.  The descriptor covers exactly the bytes of this copy: an offset past them would be dropped by the hardware.
typedef unsigned int gnms_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void w_rows_write_through(u64* dst, const u64* src, int words) {
    const unsigned bytes = (unsigned)words * 8u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)bytes, 0x00020000);   // raw buffer, 32-bit data format
    for (unsigned o = threadIdx.x * 16u; o < bytes; o += blockDim.x * 16u)
        __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const gnms_u4*>(reinterpret_cast<const char*>(src) + o), rsrc, (int)o, 0, 16);
}
// which kernels write W through (gnms_internal_launch_bitmask_boxes / gnms_internal_launch_bitmask in nms_layer.hip pass it on; w_write_through_routes there)
enum : int { kWtKbw2 = 1, kWtKbw1 = 2, kWtChunkLoop = 4, kWtMatrixIn = 8 };

template <bool VEC, int WAVES = kMaskWaves, int RB = kMaskRB>
__global__ __launch_bounds__(WAVES * 64) void bitmask_kernel(const float* __restrict__ iou, int N, long ld, const int* __restrict__ counts,
                                                                  float thr, char* ws, gnms_ws_layout L, int full, int wt) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int kb = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    const int k0 = kb * 64;
    // column chunk rotated by the row block: with pre-sorted scores half the tiles exit below, and an un-rotated grid
    // would leave that work on every other XCD (blocks are dealt round-robin to the 8 XCDs)
    const int bx = (blockIdx.x + kb) % gridDim.x;
    const int c0 = (bx * WAVES + wave) * 256;
    // `full` with ONE 16-wave workgroup per rank block (N <= 4096): the row of W is collected in LDS, by column rank, and leaves as
    // one coalesced write -- N scattered 8-byte stores per row block otherwise (the triangle alone is half of them)
    __shared__ __attribute__((aligned(16))) u64 rowbuf[(WAVES == 16) ? 4096 : 1];
    const bool rowbuffered = WAVES == 16 && full && gridDim.x == 1 && L.NC <= 4096;
    if (k0 >= n) return;                                                 // (workgroup-uniform)
    ImgPtrs I = img_ptrs(ws, L, b);
    const bool ident = I.misc[2] != 0;                                   // scores were already sorted: rank == input index
    const bool idle = c0 >= n || (ident && c0 >= k0 + 64);               // (pre-sorted: no leader of this row block lives in these columns)
    if (idle && !rowbuffered) return;
    const float* m = iou + (size_t)b * N * ld;

    const int myrank = k0 + lane;
    const int myrow = (myrank < n) ? I.order[myrank] : I.order[k0];      // clamp to a valid row; bits masked below
    const int nrows = min(64, n - k0);
    const u64 rowmask = (nrows >= 64) ? ~0ull : ((1ull << nrows) - 1ull);

    int col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = VEC ? (c0 + 4 * lane + j) : (c0 + lane + 64 * j);
    // VEC reads 16 B at col[0]; legal while col[0]+3 < ld (ld % 4 == 0).  Columns >= n produce words nobody stores.
    const bool active = VEC ? (col[0] + 3 < ld) : true;

    unsigned wd[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (!idle) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll 1
        for (int rb = 0; rb < 32; rb += RB) {
            float v[RB][4];
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int row = __builtin_amdgcn_readlane(myrow, half * 32 + rb + u);
                const float* p = m + (size_t)row * ld;
                if (VEC) {
                    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (active) t = load_nt_f4(p + col[0]);
                    v[u][0] = t.x; v[u][1] = t.y; v[u][2] = t.z; v[u][3] = t.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[u][j] = (col[j] < n) ? __builtin_nontemporal_load(p + col[j]) : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const unsigned bit = 1u << (rb + u);
#pragma unroll
                for (int j = 0; j < 4; ++j) wd[half][j] |= !(v[u][j] <= thr) ? bit : 0u;   // lib/groomed_nms.py:250 (NaN -> removed)
            }
        }
    }
    }
    // scatter each column word to the column's RANK: downstream kernels then read W contiguously
    u64* Wk = I.W + (size_t)kb * L.NC;
    int rk[4];
    if (ident) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rk[j] = col[j];
    } else if (VEC && col[3] < n) {
        const int4 t = *reinterpret_cast<const int4*>(I.rankof + col[0]);
        rk[0] = t.x; rk[1] = t.y; rk[2] = t.z; rk[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) rk[j] = (col[j] < n) ? I.rankof[col[j]] : col[j];       // (padding: rank == index)
    }
    if (rowbuffered) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 w = (col[j] < n && !idle) ? ((((u64)wd[1][j] << 32) | wd[0][j]) & rowmask) : 0ull;
            if (col[j] < L.NC && rk[j] >= 0 && rk[j] < L.NC) rowbuf[rk[j]] = w;
        }
        __syncthreads();
        if (wt) w_rows_write_through(Wk, rowbuf, L.NC);
        else for (int i = threadIdx.x; i < L.NC; i += WAVES * 64) Wk[i] = rowbuf[i];
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // only words a leader scan can read: the column must outrank some row of the block (the others are never looked at) -- or,
        // `full`, the whole row: wsym_check_kernel then decides whether the thresholded matrix is symmetric and the scan may pull
        if (col[j] < n && (full || rk[j] < k0 + 64)) Wk[rk[j]] = (((u64)wd[1][j] << 32) | wd[0][j]) & rowmask;
    }
}

// ------------------------------------------------------------------------------------------------
// K2s: is the thresholded matrix SYMMETRIC?  (matrix-in layer, round 3.)  The callers of differentiable_nms(scores, iou) hand it
// iou(boxes, boxes) -- symmetric -- but the interface does not say so, and the general scan (candidates push leader by leader: ~130
// cycles per leader on one wave) is what makes uniform boxes cost 132 us in K3 where the pulling scan of the from-boxes layer takes
// 25-30.  With the rows of W stored in full (bitmask_kernel, `full`) symmetry is a property of W alone: for every pair of rank blocks
// (kb <= jb) the 64 x 64 bit block W[kb][64 jb ..] must be the transpose of W[jb][64 kb ..].  One wave per pair: both blocks are one
// coalesced 512-byte load each, the transpose is six butterfly stages across the lanes.  The verdict lands in misc[3] (1 = not
// symmetric, or not decidable: pre-sorted scores store only the triangle); K3 / K4 read it when called with sym = 2.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 transpose64(u64 x, int lane) {            // lane r, bit c  <->  lane c, bit r
#pragma unroll
    for (int j = 32; j >= 1; j >>= 1) {
        const u64 m = j == 32 ? 0x00000000ffffffffull : j == 16 ? 0x0000ffff0000ffffull : j == 8 ? 0x00ff00ff00ff00ffull
                    : j == 4 ? 0x0f0f0f0f0f0f0f0full : j == 2 ? 0x3333333333333333ull : 0x5555555555555555ull;   // bit positions with bit j clear
        const u64 t = (u64)__shfl_xor((unsigned long long)x, j, 64);
        x = (lane & j) ? (((t >> j) & m) | (x & ~m)) : ((x & m) | ((t << j) & ~m));
    }
    return x;
}

// (round 4: no density gate any more -- with the scan on one workgroup per super-block the symmetric path is the faster one for dense
// images too)
// one pair (kb <= jb) of 64 x 64 bit blocks, pair index pr row-major over the upper triangle, by one wave: true = not each other's transpose
__device__ __forceinline__ bool wsym_pair_bad(const ImgPtrs& I, const gnms_ws_layout& L, const int n, const int nb, const int pr, const int lane) {
    auto rows_of = [&](int blk) { const int r = min(64, n - blk * 64); return r >= 64 ? ~0ull : ((1ull << r) - 1ull); };
    // pr -> (kb, jb): pairs before row kb = kb * nb - kb (kb - 1) / 2
    const float a = (float)(2 * nb + 1);
    int kb = (int)((a - sqrtf(a * a - 8.0f * (float)pr)) * 0.5f);
    kb = kb < 0 ? 0 : (kb >= nb ? nb - 1 : kb);
    while (kb > 0 && kb * nb - kb * (kb - 1) / 2 > pr) --kb;
    while ((kb + 1) * nb - (kb + 1) * kb / 2 <= pr) ++kb;
    const int jb = kb + (pr - (kb * nb - kb * (kb - 1) / 2));
    // A: rows = ranks of block kb (bits), columns = ranks of block jb (lanes); Bm the other way round
    const u64 A = (jb * 64 + lane < n) ? (I.W[(size_t)kb * L.NC + jb * 64 + lane] & rows_of(kb)) : 0ull;
    const u64 Bm = (kb * 64 + lane < n) ? (I.W[(size_t)jb * L.NC + kb * 64 + lane] & rows_of(jb)) : 0ull;
    return A != transpose64(Bm, lane);
}

// The same check as a ROLE of the tail launch (round 5, the matrix-in layer with the fast tail): workgroup `wg` of `nwg` checker workgroups
// (the FIRST workgroups of the grid: they wait for nobody) takes every nwg-th group of 16 pairs of every image, while the chain workgroups
// already run the symmetric scan on the assumption that the check will pass; the image's last chain workgroup waits for the verdict --
// misc[7] == nwg workgroups done, misc[3] != 0: some pair failed -- before anything is final, and falls back to the general scan if it has to.
// (As a launch of its own the check cost 9.9 us in front of the tail, B = 8, N = 4096.)  Images whose scores came in sorted (misc[2]: W
// holds the triangle only) are not checked at all: everybody reads misc[2] and takes the general scan.
__device__ __forceinline__ void wsym_check_in_launch(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, const int B, const int wg,
                                                     const int nwg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int b = 0; b < B; ++b) {
        const int n = gnms_count(counts, b, N);
        ImgPtrs I = img_ptrs(ws, L, b);
        if (I.misc[2] != 0) continue;
        const int nb = (n + 63) >> 6;
        const int pairs = nb * (nb + 1) / 2;
        bool bad = false;
        for (int pr = wg * nw + wave; pr < pairs; pr += nwg * nw) bad |= wsym_pair_bad(I, L, n, nb, pr, lane);
        if (__any(bad) && lane == 0) __hip_atomic_store(I.misc + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0x0f70);                              // vmcnt(0): the flag is out before this workgroup counts as done
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(I.misc + 7, 1);
    }
}

// ------------------------------------------------------------------------------------------------
// K2b: threshold bit matrix straight from the boxes (the from-boxes path: no read of the N x N fp32 matrix).
// Wave tile = 64 rank-rows (block kb) x 256 columns; the overlap of each pair is recomputed from the two boxes and
// thresholded in registers, bit-identical to thresholding the matrix.  Bound: fp32 VALU; HBM traffic is 16 N bytes in
// and <= N^2/8 bytes out per image.
// ------------------------------------------------------------------------------------------------
// Columns in X ORDER + row culling.
// The column a lane owns only decides WHICH word it writes (W[kb][rank of the column]); the order in which columns are
// dealt to lanes is free.  Dealing them by ascending x centre (sort_boxes_by_x) makes the 256 columns of a wave tile
// spatial neighbours: their hull is a narrow strip of the image, and a row box that does not reach into the hull has
// intersection 0 with all 256 columns -> its bit is 0 in every word and the row is skipped (exact: with finite positive
// areas and thr >= 0, inter = +0 and uni > 0 give 0 <= thr).  On detector-like inputs (boxes ~100 px on a 1760 px wide
// canvas) a tile keeps 15-20 % of its 64 rows.  The price: the rank triangle can no longer be skipped per tile (a tile
// holds columns of every rank); words no leader scan reads (column rank >= 64 (kb+1)) are computed but not stored.

// CPL = columns per lane: 4 (wave tile 64 x 256) when there are plenty of tiles, 1 (64 x 64) for small problems, where the 64-row
// chain of a wave is the critical path and four times as many waves share it.
// KBW = rank blocks per wave: 1, or 4 for large images (the column side -- gathers, ranks, hull -- is then paid once per 256 rows
// instead of once per 64: at N=16384 a tile keeps ~6 of its 64 rows, so that fixed part dominated).
// ROWBUF (N <= 4096, KBW = 1): the workgroup is 16 waves = ALL column chunks of ONE rank block; the words go to an LDS copy of the
// row W[kb][.] (indexed by column rank) and leave as one coalesced write of the 64 (kb+1) words a leader scan can read.  Without it
// every lane scatters its 8-byte words to global memory: 1 M scattered stores per launch at B=8, N=4096 = ~15 us of store
// throughput, about a third of it exposed.
// CHUNKLOOP (ROWBUF, N > 4096): a wave walks the column chunks wave, wave + 16, ... of its rank block (at N = 16384 four of them), all
// into the one LDS row of N words (128 KiB), which then leaves as one coalesced write: since round 2 the rows of W are stored in full
// (the scan pulls), so the scatter version issues N^2 / 64 scattered 8-byte stores per image -- 256 MB per step at B = 8, N = 16384.
template <int CPL, int KBW, bool ROWBUF, bool CHUNKLOOP = false>
__device__ __forceinline__ void bitmask_boxes_body(const float* __restrict__ boxes, int N, const int* __restrict__ counts, float thr, char* ws,
                                                   gnms_ws_layout L, const int b, const int bx, const int wt = 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = gnms_count(counts, b, N);
    constexpr int kCols = 64 * CPL;
    const int nchunk = (N + kCols - 1) / kCols;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* rowbuf = reinterpret_cast<u64*>(smem);                       // ROWBUF: [NC] words of row kb, by column rank
    ImgPtrs I = img_ptrs(ws, L, b);
#ifdef GNMS_TIMING   // developer (tools/bits_ticks.py): phase ticks of wave 0 / wave 15 of rank block 32 of image 0, into xsol
    long long bt__[6]; int bti__ = 0;
#define GNMS_BT() do { bt__[bti__++] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define GNMS_BT() do {} while (0)
#endif
    GNMS_BT();
#ifdef GNMS_TIMING
    const long long rt0__ = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    // ROWBUF with KBW = 2 (round 6; B = 8, N = 4096): a workgroup takes TWO rank blocks, their rows of W side by side in LDS.  With one
    // block per workgroup the launch was 512 workgroups, two per CU, each pulling all 4096 column boxes, their indices and ranks (96 KiB)
    // through the CU for ~3 us of arithmetic: 48 MB of L2 -> CU traffic in the first microseconds, the late waves' loads 6-8 us behind, and
    // the CU's second workgroup (younger waves) finishing 7-8 us after the first (profiles/r06j_bits_timeline.txt: image 0 done at 15 us,
    // image 7 at 23).  256 workgroups of two blocks pull half the bytes and have their CU to themselves.
    // LATE (round 7; the two-block route): the dependent gather rankof[xidx[p]] -- 64 distinct lines per instruction, the slow one -- is off the
    // path to the rows.  A wave requests its row boxes, column boxes and the columns' x-order indices, computes the hull when the boxes are
    // there, issues the gather BEHIND the hull (every wave's box loads are then in front of it in the texture pipe's queue) and waits for it only
    // where the first finished word is parked, one rows loop later: a column's rank says nothing but WHICH word of the LDS row that is.  The
    // four ranks stay in registers (one workgroup per CU: 128 VGPRs); the stash and its 16 KiB of LDS are gone here.  24.0 -> 22.2 us.
    // (KBW = 1 stays as it was: at its 64 VGPRs the same order spills 11 registers where the stash version spills 3.  Measured and not kept,
    // LABNOTES R7: the LDS rows zeroed behind the issue of the loads; the row write-out from column 64 kb on.)
    constexpr bool LATE = ROWBUF && !CHUNKLOOP && KBW > 1;
    if (ROWBUF) {
        const int kbr = bx * KBW;                             // KBW rank blocks per workgroup, wave w = column chunk w
        if (kbr * 64 >= n) return;
        for (int i = threadIdx.x; i < KBW * L.NC; i += blockDim.x) rowbuf[i] = 0ull;
        __syncthreads();
    }
    GNMS_BT();
    const int nwaves = blockDim.x >> 6;
    for (int cq = 0; cq < (CHUNKLOOP ? (nchunk + nwaves - 1) / nwaves : 1); ++cq) {
    const int tile = ROWBUF ? bx * nchunk + wave : bx * 4 + wave;
    const int kbg = ROWBUF ? bx : tile / nchunk;        // kbg = group of KBW consecutive rank blocks
    const int chunk = ROWBUF ? wave + cq * nwaves : tile - kbg * nchunk;   // ROWBUF: one chunk per wave (CHUNKLOOP: every 16th)
    const int c0 = chunk * kCols;
    const bool idle = (kbg * KBW >= L.NB || kbg * KBW * 64 >= n || c0 >= n || chunk >= nchunk);   // (ragged images)
    if (!ROWBUF && idle) return;
    float4 rb_next;
    float4 cb[CPL];
    float carea[CPL];
    int crank[CPL];
    bool cok = true;
    if (LATE) {
        // (no branch around the requests: a wave without columns -- ragged images -- reads clamped duplicates like the lanes past the last
        // column; under `if (!idle)` the values are merged with the idle path's behind the loads, which waits for every one of them here)
        rb_next = I.rbox[min(kbg * KBW * 64 + lane, n - 1)];
#pragma unroll
        for (int j = 0; j < CPL; ++j) cb[j] = I.xbox[min(c0 + 64 * j + lane, n - 1)];
#pragma unroll
        for (int j = 0; j < CPL; ++j) crank[j] = I.xidx[min(c0 + 64 * j + lane, n - 1)];   // (the x-order index; its rank below)
    }
    if (!idle) {                                                     // (a chunk LOOP here cost 25 % in code quality at N = 4096: 24.5 -> 31 us)
    if (LATE) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            carea[j] = (cb[j].z - cb[j].x) * (cb[j].w - cb[j].y);
            cok &= (carea[j] > 0.0f) && (carea[j] < INFINITY);
        }
    } else {
    // the row boxes of the first rank block are requested before the column side is worked on
    rb_next = I.rbox[min(kbg * KBW * 64 + lane, n - 1)];            // (rank order, written by the score sort: no order -> box gather)
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        // (round 6: column 64 j + lane, not CPL lane + j.  With four CONSECUTIVE columns per lane the lanes of one load instruction sat 64 bytes
        // apart -- 64 requests to the texture pipe per instruction, four instructions over the same lines -- and the sixteen waves' column
        // phases queued behind each other at ~0.7 k ticks a wave (wave 0: 8 k, wave 15: 18 k, profiles/r06k_bits_timeline.txt); which lane
        // holds which column is free: the word goes to the column's rank)
        const int p = c0 + 64 * j + lane;
        const int pp = p < n ? p : n - 1;                             // clamped duplicates: harmless in the hull, never stored
        cb[j] = I.xbox[pp];
        crank[j] = (p < n) ? I.rankof[I.xidx[pp]] : 0x7fffffff;
        carea[j] = (cb[j].z - cb[j].x) * (cb[j].w - cb[j].y);
        cok &= (carea[j] > 0.0f) && (carea[j] < INFINITY);
    }
    }
    // Decision !(fl(inter/uni) <= thr) WITHOUT the division: the sign of d = fma(-thr, uni, inter) outside the guard band (iou_guard_band,
    // gnms_device.h: why 8 ulp suffice).  Positive finite areas are checked once per column box and per row; rows/columns that fail, and
    // the pairs inside the guard band, take the exact IEEE division.
    // (KBW = 1: two workgroups per CU leave 64 VGPRs: the columns' ranks, not needed before the words are parked, wait in LDS meanwhile.
    // KBW = 2 is one workgroup per CU with 128 VGPRs: the four ranks stay in registers, their gather in flight behind the first rows loop)
    constexpr bool STASH = ROWBUF && !CHUNKLOOP && CPL == 4 && KBW == 1;
    int* const crank_lds = reinterpret_cast<int*>(smem + (size_t)KBW * L.NC * 8) + threadIdx.x;   // [CPL][1024] (behind the KBW rows)
    if (STASH) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) crank_lds[j * 1024] = crank[j];
    }
    const float guard = iou_guard_band(thr);
    const bool cols_ok = __all(cok);
    const bool plain_img = I.misc[6] == 0;                            // (sort_boxes_by_x / sort_merge_body: no box that is not plain)
    // hull of the tile's columns
    float hx0 = cb[0].x, hx1 = cb[0].z, hy0 = cb[0].y, hy1 = cb[0].w;
#pragma unroll
    for (int j = 1; j < CPL; ++j) { hx0 = fminf(hx0, cb[j].x); hx1 = fmaxf(hx1, cb[j].z); hy0 = fminf(hy0, cb[j].y); hy1 = fmaxf(hy1, cb[j].w); }
    hx0 = wave_min_f(hx0); hy0 = wave_min_f(hy0); hx1 = wave_max_f(hx1); hy1 = wave_max_f(hy1);
    const bool cull = cols_ok && (thr >= 0.0f);
    if (LATE) {
        // the gather goes out BEHIND the hull (the sixteen waves' box loads are all in front of it in the texture pipe's queue) and is in flight
        // during the first rows loop; clamped duplicates included: they are not parked, see `live` below
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < CPL; ++j) crank[j] = I.rankof[crank[j]];
    }
    GNMS_BT();
#pragma unroll 1
    for (int kw = 0; kw < KBW; ++kw) {
        const int kb = kbg * KBW + kw;
        const int k0 = kb * 64;
        if (kb >= L.NB || k0 >= n) break;
        const float4 rb = rb_next;
        if (KBW > 1 && kw + 1 < KBW && kb + 1 < L.NB && k0 + 64 < n) rb_next = I.rbox[min(k0 + 64 + lane, n - 1)];   // next block's rows
        const float rarea = (rb.z - rb.x) * (rb.w - rb.y);
        const int nrows = min(64, n - k0);
        const bool row_fine = (rarea > 0.0f) && (rarea < INFINITY);
        const u64 rows_ok = __ballot(row_fine);
        // the rows that reach into the hull
        const bool reaches = (rb.z > hx0) && (rb.x < hx1) && (rb.w > hy0) && (rb.y < hy1);
        const u64 active = __ballot((lane < nrows) && (!(cull && row_fine) || reaches));
        unsigned wd[2][CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) { wd[0][j] = 0u; wd[1][j] = 0u; }
        // PLAIN images (misc[6] == 0: every box finite, x2 >= x1, y2 >= y1, no negative zero; decided by the x sort): the intersection
        // as iou_tile.h derives it -- w = med3(min3(fl(ax2 - bx1), fl(bx2 - ax1), cw), 0, rw), bit for bit the reference's
        // relu(min - max) -- packed over column pairs, and the decided bit taken from the SIGN of thr * uni - inter (an arithmetic shift
        // and one v_and_or per entry instead of compare, select, or): 11.5 VALU slots per entry instead of 17.
        bool fast_rows = false;
        if constexpr (CPL == 4) fast_rows = plain_img && cols_ok && rows_ok == ~0ull;   // (lanes past the last row hold copies of it)
        if constexpr (CPL == 4) if (fast_rows) {
            using gnms_iou::gnms_f2;
            gnms_f2 cx1[2], cy1[2], cx2[2], cy2[2], cw[2], ch[2], ca[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cx1[j >> 1][j & 1] = cb[j].x; cy1[j >> 1][j & 1] = cb[j].y; cx2[j >> 1][j & 1] = cb[j].z; cy2[j >> 1][j & 1] = cb[j].w;
                cw[j >> 1][j & 1] = cb[j].z - cb[j].x; ch[j >> 1][j & 1] = cb[j].w - cb[j].y;
                ca[j >> 1][j & 1] = carea[j];
            }
            const float rw = rb.z - rb.x, rh = rb.w - rb.y;
            const gnms_f2 sthr = {thr, thr}, sguard = {guard, guard};
            // one row against the lane's four columns: nd = thr * uni - inter (its sign decides), true if some pair lies in the guard band
            auto row_core = [&](int r, gnms_f2 (&inter)[2], gnms_f2 (&uni)[2], gnms_f2 (&nd)[2]) -> bool {
                const float ax1 = gnms_iou::bcast(rb.x, r), ay1 = gnms_iou::bcast(rb.y, r), ax2 = gnms_iou::bcast(rb.z, r), ay2 = gnms_iou::bcast(rb.w, r);
                const float aw = gnms_iou::bcast(rw, r), ah = gnms_iou::bcast(rh, r), aa = gnms_iou::bcast(rarea, r);
                const gnms_f2 sx1 = {ax1, ax1}, sy1 = {ay1, ay1}, sx2 = {ax2, ax2}, sy2 = {ay2, ay2}, sa = {aa, aa};
                bool unsure = false;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const gnms_f2 dx1 = sx2 - cx1[p], dx2 = cx2[p] - sx1;
                    const gnms_f2 dy1 = sy2 - cy1[p], dy2 = cy2[p] - sy1;
                    const gnms_f2 w = {gnms_iou::hw_clamp0_s(gnms_iou::hw_min3(dx1.x, dx2.x, cw[p].x), aw),
                                       gnms_iou::hw_clamp0_s(gnms_iou::hw_min3(dx1.y, dx2.y, cw[p].y), aw)};
                    const gnms_f2 h = {gnms_iou::hw_clamp0_s(gnms_iou::hw_min3(dy1.x, dy2.x, ch[p].x), ah),
                                       gnms_iou::hw_clamp0_s(gnms_iou::hw_min3(dy1.y, dy2.y, ch[p].y), ah)};
                    inter[p] = w * h;
                    uni[p] = (sa + ca[p]) - inter[p];                     // row box is `a`, column (leader) box is `b`
                    nd[p] = __builtin_elementwise_fma(sthr, uni[p], -inter[p]);   // = -fma(-thr, uni, inter) exactly (one rounding either way)
                    const gnms_f2 g = sguard * uni[p];
                    unsure |= !(fabsf(nd[p].x) > g.x) || !(fabsf(nd[p].y) > g.y);   // also true for NaN
                }
                return __any(unsure);
            };
            // The loop over the surviving rows is BRANCH-FREE, two rows per trip: every bit is taken from the sign of nd, the rows
            // with a pair in the guard band are only noted (`redo`) and re-decided with the IEEE division behind the loop.  The kernel
            // is bound by its slowest waves (dense x stretches keep 3x the rows of the mean), not by VALU throughput: what counts
            // is the latency of ONE wave's row chain, and two independent rows in flight shorten it.
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                unsigned todo = (unsigned)(half ? (active >> 32) : (active & 0xffffffffull));
                unsigned redo = 0u;
                while (todo) {                                        // wave-uniform
                    const int r0 = __builtin_ctz(todo);
                    todo &= todo - 1u;
                    const int r1 = todo ? __builtin_ctz(todo) : r0;   // (odd count: the last row twice -- the same bits again)
                    todo &= todo - 1u;                                // (0 stays 0)
                    gnms_f2 i0[2], u0[2], n0[2], i1[2], u1[2], n1[2];
                    const bool q0 = row_core(half * 32 + r0, i0, u0, n0);
                    const bool q1 = row_core(half * 32 + r1, i1, u1, n1);
                    const unsigned b0 = 1u << r0, b1 = 1u << r1;
                    redo |= (q0 ? b0 : 0u) | (q1 ? b1 : 0u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {                     // decided pairs: d = -nd != 0, the bit is "nd negative"
                        wd[half][j] |= (unsigned)(__float_as_int(n0[j >> 1][j & 1]) >> 31) & b0;
                        wd[half][j] |= (unsigned)(__float_as_int(n1[j >> 1][j & 1]) >> 31) & b1;
                    }
                }
                while (redo) {                                        // rare: a few rows per image
                    const int rr = __builtin_ctz(redo);
                    redo &= redo - 1u;
                    gnms_f2 ii[2], uu[2], nn[2];
                    row_core(half * 32 + rr, ii, uu, nn);
                    const unsigned bit = 1u << rr;
#pragma unroll
                    for (int j = 0; j < 4; ++j) wd[half][j] = (wd[half][j] & ~bit) | (!(ii[j >> 1][j & 1] / uu[j >> 1][j & 1] <= thr) ? bit : 0u);
                }
            }
        }
        if (!fast_rows) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            unsigned todo = (unsigned)(half ? (active >> 32) : (active & 0xffffffffull));
            while (todo) {                                            // wave-uniform loop over the surviving rows
                const int rr = __builtin_ctz(todo);
                todo &= todo - 1u;
                const int r = half * 32 + rr;
                const float ax1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rb.x), r));
                const float ay1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rb.y), r));
                const float ax2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rb.z), r));
                const float ay2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rb.w), r));
                const float aa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rarea), r));
                const unsigned bit = 1u << rr;
                float inter4[CPL], uni4[CPL], d4[CPL];
                bool unsure = false;
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    iou_row_terms(ax1, ay1, ax2, ay2, aa, cb[j], carea[j], thr, inter4[j], uni4[j], d4[j]);
                    unsure |= !(fabsf(d4[j]) > guard * uni4[j]);          // also true for NaN
                }
                if (!(cols_ok && ((rows_ok >> r) & 1ull)) || __any(unsure)) {
#pragma unroll
                    for (int j = 0; j < CPL; ++j) wd[half][j] |= !(inter4[j] / uni4[j] <= thr) ? bit : 0u;
                } else {
#pragma unroll
                    for (int j = 0; j < CPL; ++j) wd[half][j] |= (d4[j] > 0.0f) ? bit : 0u;
                }
            }
        }
        }   // !fast_rows
        // the FULL row of W: the overlap is symmetric, and with all columns present the leader scan can pull (leaders_body, sym)
        u64* Wk = ROWBUF ? rowbuf + (size_t)kw * L.NC : I.W + (size_t)kb * L.NC;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int cr = STASH ? crank_lds[j * 1024] : crank[j];
            const bool live = LATE ? (c0 + 64 * j + lane < n) : (cr != 0x7fffffff);
            if (live) Wk[cr] = ((u64)wd[1][j] << 32) | wd[0][j];
        }
    }
    }   // !idle
    }   // chunks of this wave
    GNMS_BT();
    if (ROWBUF) {
        __syncthreads();
        GNMS_BT();
        if (wt) {                                                      // (wave-uniform: a kernel argument)
            // the rows of the workgroup's live rank blocks as ONE span, written through (w_rows_write_through); block bx * KBW is live here
            int live = 1;
            while (live < KBW && bx * KBW + live < L.NB && (bx * KBW + live) * 64 < n) ++live;
            w_rows_write_through(I.W + (size_t)bx * KBW * L.NC, rowbuf, live * L.NC);
        } else
        for (int kw = 0; kw < KBW; ++kw) {
            const int kb = bx * KBW + kw;
            if (kb >= L.NB || kb * 64 >= n) break;
            u64* Wk = I.W + (size_t)kb * L.NC;
            for (int i = threadIdx.x; i < L.NC; i += blockDim.x) Wk[i] = rowbuf[(size_t)kw * L.NC + i];   // the whole row, coalesced
        }
    }
    GNMS_BT();
#ifdef GNMS_TIMING
    if (ROWBUF && !CHUNKLOOP && b == 0 && bx == (int)gridDim.x / 2 && (threadIdx.x == 0 || threadIdx.x == 960)) {
        long long* o = reinterpret_cast<long long*>(I.xsol) + (threadIdx.x ? 8 : 0);
        for (int q = 1; q < 6; ++q) o[q] += bt__[q] - bt__[q - 1];
    }
    // (round 6) the launch's timeline: every workgroup's start and end on the constant-rate clock (s_memrealtime, 100 MHz, one clock for all
    // XCDs), last call only -- tools/bits_ticks.py
    if (ROWBUF && !CHUNKLOOP && threadIdx.x == 0 && bx < 256) {
        long long* o = reinterpret_cast<long long*>(I.xsol) + 32 + 2 * bx;
        o[0] = rt0__; o[1] = (long long)__builtin_amdgcn_s_memrealtime();
    }
#endif
}

// (ROWBUF without the chunk loop: two 16-wave workgroups per CU = 8 waves per SIMD, i.e. at most 64 VGPRs -- asked for explicitly)
template <int CPL, int KBW, bool ROWBUF = false, bool CHUNKLOOP = false>
__global__ __launch_bounds__(ROWBUF ? 1024 : 256, (ROWBUF && !CHUNKLOOP) ? (KBW > 1 ? 4 : 8) : 1) void bitmask_boxes_kernel(const float* __restrict__ boxes, int N, const int* __restrict__ counts,
                                                            float thr, char* ws, gnms_ws_layout L, int wt) {
    bitmask_boxes_body<CPL, KBW, ROWBUF, CHUNKLOOP>(boxes, N, counts, thr, ws, L, (int)blockIdx.z, (int)blockIdx.x, wt);
}

// The scatter variant (no LDS row) with the row groups dealt to the XCDs, as bitmask_rec3d_culled_kernel does (round 4b): workgroup x runs on
// XCD x mod 8, its four waves are four consecutive column chunks of one row group, consecutive workgroups of an XCD walk the chunks of a
// row group -- every row of W is completed in ONE L2.  Needs a whole number of workgroups per row group (N a multiple of 1024).
template <int KBW>
__global__ __launch_bounds__(256) void bitmask_boxes_pinned_kernel(const float* __restrict__ boxes, int N, const int* __restrict__ counts, float thr,
                                                                   char* ws, gnms_ws_layout L) {
    const int wpk = ((N + 255) >> 8) >> 2;                           // workgroups per row group
    const int x = (int)blockIdx.x, s = x >> 3;
    const int kbg = (s / wpk) * 8 + (x & 7);
    bitmask_boxes_body<4, KBW, false, false>(boxes, N, counts, thr, ws, L, (int)blockIdx.z, kbg * wpk + (s % wpk));
}

// ------------------------------------------------------------------------------------------------
// K2c: threshold bit matrix of the 3D NMS overlap straight from the cuboid records (gnms_forward_with_iou3d: the matrix is an
// output, the layer does not read it back).  Wave tile = 64 rank-rows x 256 RANK columns (records gathered through `order`);
// every pair runs gnms_iou3d::nms_overlap3d -- the very instruction sequence iou3d_nms_fast_kernel wrote the matrix with -- and
// is thresholded in registers: the same bits as bitmask_kernel on that matrix.  Only tiles a leader can reach (column chunk
// below the end of the row block) exist; they are numbered in one dimension so that every wave has equal work.
// Bound: fp32 VALU, ~29 slots per pair on N^2/2 pairs.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tri_tile(int id, int* kb, int* chunk) {     // tiles before row block kb = 4q + r:  2q(q+1) + r(q+1)
    int q = (int)((sqrtf(1.0f + 2.0f * (float)id) - 1.0f) * 0.5f);
    while (2 * q * (q + 1) > id) --q;
    while (2 * (q + 1) * (q + 2) <= id) ++q;
    const int rem = id - 2 * q * (q + 1);
    const int r = rem / (q + 1);
    *kb = 4 * q + r;
    *chunk = rem - r * (q + 1);
}
__host__ __device__ inline int tri_tile_count(int NB) {                // number of reachable tiles for NB row blocks
    const int q = NB >> 2, r = NB & 3;
    return 2 * q * (q + 1) + r * (q + 1);
}

// K2c with spatially ordered columns and row culling (the 3D counterpart of bitmask_boxes_kernel).  For GIoU a DISJOINT pair can
// still exceed the threshold, so "does not reach the hull" is not enough; what holds for two boxes separated along an axis (x or z) by
// a gap g >= 0 is
//     i3 = 0,   q = u3 / (2 vh),   u3 = vol_a + vol_b <= (lx_a + lx_b) * max(ly) * max(lz),   vh >= (lx_a + lx_b + g) * max(ly) * max(lz)
//     =>  q <= (lx_a + lx_b) / (2 (lx_a + lx_b + g))  <=  thr     as soon as     g >= (lx_a + lx_b) * (1 / (2 thr) - 1).
// A row is skipped against a set of columns when its gap to the set's hull satisfies that with the set's largest extent and an ADDITIVE
// 1e-3 on the factor (relative margin 2e-3 thr on q: three orders above the fp32 rounding of the matrix kernel, so the thresholded matrix
// has a 0 there too).  Needs finite positive extents on both sides and thr >= 0.01; everything else is evaluated.
// Round 4b: the cull works per SLOT.  The columns come in (z band, x centre) order (column_key; records in that order: xrec), a wave tile
// is 4 slots of 64 consecutive columns (lane l holds column 64 j + l of slot j), each slot a compact patch in x and z with its own hulls,
// and a row is evaluated only against the slots it can reach -- one column wide (nms_overlap3d_guarded1: v_pk_* run at the scalar rate on
// gfx950, so four single evaluations cost what two packed ones did).  With one x-ordered 256-column hull per tile 27 % of the (row, tile)
// pairs survived at N = 4096 (the gap bound lets boxes ~4 units apart through, the scene is 60 x 55); per slot ~12 % do.
// Tile numbering.  A tile scatters its 256 words over a whole row of W (column p goes to word rank(p)); what completes the 64-byte lines
// is the L2.  `pinned` (N > 4096: rows of >= 64 KiB): the row groups are dealt to the XCDs (workgroup x runs on XCD x mod 8; the four waves of
// a workgroup are four consecutive chunks of one row group, consecutive workgroups of an XCD walk the chunks of a row group), so that every
// row is written through ONE L2 by workgroups that run together: B = 8, N = 16384 409 -> 331 us, 8192 135 -> 129.  Otherwise ROW GROUP
// FASTEST (round 4): what a tile costs is set by its column chunk, hardly by its row group (ranks are spatially random); numbered chunk-fastest
// the heavy tiles of an image recurred on one or two XCDs, where they queued eight deep per CU while the others ran dry (LABNOTES.md 3.2c).
// (Persistent waves claiming tiles from a counter, round 4b: 75 us instead of 46 at N = 4096, 481 instead of 409 at 16384 -- ~1 700 claims
// per image on one address serialise in the memory-side atomic unit; LABNOTES R4b.)
template <int KBW>
__global__ __launch_bounds__(256) void bitmask_rec3d_culled_kernel(int N, const int* __restrict__ counts, float thr, char* ws, gnms_ws_layout L, int pinned) {
    using namespace gnms_iou3d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int n = gnms_count(counts, b, N);
    const int nchunk = (N + 255) >> 8;
    const int nkbg = (L.NB + KBW - 1) / KBW;
    int chunk, kbg;
    if (pinned) {
        const int wpk = (nchunk + 3) >> 2, x = blockIdx.x, s = x >> 3;
        kbg = (s / wpk) * 8 + (x & 7);
        chunk = (s % wpk) * 4 + wave;
    } else {
        const int tile = blockIdx.x * 4 + wave;
        chunk = tile / nkbg;
        kbg = tile - chunk * nkbg;
    }
    const int c0 = chunk * 256;
    if (chunk >= nchunk || kbg >= nkbg || kbg * KBW >= L.NB || kbg * KBW * 64 >= n || c0 >= n) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    const bool thr_ok = (thr >= 0.01f) && (thr < INFINITY);
    const float kappa = fmaxf(1.0f / (2.0f * thr) - 1.0f, 0.0f) + 1e-3f;
    {
    Col1 col[4];
    int crank[4];
    bool colbad[4], sane[4], cullj[4];
    float hx0[4], hx1[4], mlx[4], hz0[4], hz1[4], mlz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = c0 + 64 * j + lane;
        const int pp = p < n ? p : n - 1;
        const float4* rp = reinterpret_cast<const float4*>(I.xrec) + (size_t)pp * 3;
        const float4 u = rp[0], v = rp[1], e = rp[2];
        col1_set(col[j], u, v, e);
        colbad[j] = e.w != 0.0f;
        crank[j] = (p < n) ? I.rankof[I.xidx[pp]] : 0x7fffffff;
        const bool cok = (e.x > 0.0f) && (e.y > 0.0f) && (e.z > 0.0f) && (u.x > 0.0f) && (u.x < INFINITY);   // extents and volume positive, finite
        hx0[j] = wave_min_f(u.w); hx1[j] = wave_max_f(v.x); mlx[j] = wave_max_f(e.x);
        hz0[j] = wave_min_f(v.y); hz1[j] = wave_max_f(v.z); mlz[j] = wave_max_f(e.z);
        cullj[j] = __all(cok) && thr_ok;
        sane[j] = __all(!colbad[j]);
    }
#pragma unroll 1
    for (int kw = 0; kw < KBW; ++kw) {
        const int kb = kbg * KBW + kw;
        const int k0 = kb * 64;
        if (kb >= L.NB || k0 >= n) break;
        const float4* rp = reinterpret_cast<const float4*>(I.rec + (size_t)I.order[min(k0 + lane, n - 1)] * kRec);
        const float4 ru = rp[0], rv = rp[1], re = rp[2];
        const int nrows = min(64, n - k0);
        const bool row_fine = (re.x > 0.0f) && (re.y > 0.0f) && (re.z > 0.0f) && (ru.x > 0.0f) && (ru.x < INFINITY);
        u64 act[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gap = fmaxf(hx0[j] - rv.x, ru.w - hx1[j]);    // >= 0: the row box lies beside the slot's hull (x0 = ru.w, x1 = rv.x)
            const float gapz = fmaxf(hz0[j] - rv.z, rv.y - hz1[j]);   // z0 = rv.y, z1 = rv.z
            const bool skip = cullj[j] && row_fine && (((gap >= 0.0f) && (gap >= (re.x + mlx[j]) * kappa)) ||
                                                       ((gapz >= 0.0f) && (gapz >= (re.z + mlz[j]) * kappa)));
            act[j] = __ballot((lane < nrows) && !skip);
        }
        const u64 any = (act[0] | act[1]) | (act[2] | act[3]);
        unsigned wd[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            unsigned todo = (unsigned)(half ? (any >> 32) : (any & 0xffffffffull));
            while (todo) {
                const int rr = __builtin_ctz(todo);
                todo &= todo - 1u;
                const int r = half * 32 + rr;
                auto bc = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); };
                Row a;
                a.vol = bc(ru.x); a.y0 = bc(ru.y); a.y1 = bc(ru.z); a.x0 = bc(ru.w); a.x1 = bc(rv.x); a.z0 = bc(rv.y); a.z1 = bc(rv.z);
                a.lx = bc(re.x); a.ly = bc(re.y); a.lz = bc(re.z); a.bad = bc(re.w);
                const unsigned bit = 1u << rr;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((act[j] >> r) & 1ull) {                        // wave-uniform
                        const float q = nms_overlap3d_guarded1(a, col[j], colbad[j], sane[j], thr);
                        wd[half][j] |= !(q <= thr) ? bit : 0u;
                    }
                }
            }
        }
        u64* Wk = I.W + (size_t)kb * L.NC;                             // full rows (symmetric overlap): see bitmask_boxes_kernel
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (crank[j] != 0x7fffffff) Wk[crank[j]] = ((u64)wd[1][j] << 32) | wd[0][j];
        }
    }
    }
}

// (Round 3 tried this kernel with the LDS row buffer that won for the 2D boxes at large N -- one 16-wave workgroup per rank block, the
// full row of W written coalesced: at 106 VGPRs only one such workgroup fits a CU and the record gathers of the column side are exposed:
// B = 8, N = 16384 step 2.20 -> 2.33 ms, N = 8192 0.593 -> 0.616.  The scatter kernel stays.)

// ------------------------------------------------------------------------------------------------
// K4: attribution.  One wave per rank block: walk the leaders with rank < 64(kb+1) in order, 64 per step;
// an exclusive OR-scan across lanes tells each leader which bits it is the FIRST to claim.
//   rem[k] = rank of the leader that removed rank k (k itself for a leader), gpos[k] = that leader's ordinal.
// ------------------------------------------------------------------------------------------------
// one wave: rank block kb of image b.  Besides the attribution it evaluates, in parallel over all rank blocks, the overlap of
// every rank with the leader that removed it (plead[k], groups_kernel's membership test) -- as a prologue of groups_kernel these
// N dependent gathers ran on ONE CU (50 us of its 180 at N=16384).  `src`: see kFromMatrix / kFromBoxes / kFromRecords.
template <int SRC>
__device__ __forceinline__ void attribute_body(const float* __restrict__ src, long ld, int N, const int* __restrict__ counts, float thr, char* ws,
                                               gnms_ws_layout L, const int b, const int kb, const int lane, const int sym_arg = 0) {
    __shared__ int att_lead[16][64];                   // per wave: ordinal of the leader that claimed rank k0 + i
    int* my_lead = att_lead[(threadIdx.x >> 6) & 15];
    const int n = gnms_count(counts, b, N);
    const int k0 = kb << 6;
    if (k0 >= n) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    const int sym = sym_arg == 2 ? (I.misc[3] == 0 ? 1 : 0) : sym_arg;  // (2: wsym_check_kernel's verdict)
    const int nrows = min(64, n - k0);
    const u64 want = (nrows >= 64) ? ~0ull : ((1ull << nrows) - 1ull);
    const u64* slab = I.W + (size_t)kb * L.NC;
    const int nl = I.leadpfx[kb + 1];                 // leaders with rank < k0 + 64
    my_lead[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    u64 acc = 0;
    if (sym) {
        // the leader scan has attributed already (leaders_body, sym): rem[k] is final, what is left is the leader's ordinal and the
        // overlap with it
        if (lane < nrows) {
            const int k = k0 + lane;
            const int lr = rem_load(I.rem, k);
            const int g = I.leadpfx[lr >> 6] + __builtin_popcountll(I.leadw[lr >> 6] & ((1ull << (lr & 63)) - 1ull));
            I.gpos[k] = g;
            const float* m = overlap_src<SRC>(src, I, b, N, ld);
            I.plead[k] = overlap_at<SRC>(m, ld, I.order[k], I.leadc[g], thr);
        }
        return;
    }
    for (int base = 0; base < nl && (acc & want) != want; base += 64) {
        const int t = base + lane;
        u64 w = 0;
        int lr = -1;
        if (t < nl) {
            lr = I.leadr[t];
            w = slab[lr];
            if (lr >= k0) w |= 1ull << (lr - k0);     // the leader's own slot
            w &= want;
        }
        const u64 ex = wave_or_exclusive_scan(w, lane);
        u64 mine = w & ~(acc | ex);
        while (mine) {
            const int bit = __builtin_ctzll(mine);
            I.rem[k0 + bit] = lr;
            my_lead[bit] = t;
            mine &= mine - 1;
        }
        acc |= gnms_wave_or(w);
    }
    __builtin_amdgcn_wave_barrier();                  // LDS is in order within a wave: every claimed slot is visible below
    if (lane < nrows) {
        const int k = k0 + lane;
        const int g = my_lead[lane];                  // every rank is claimed: by an earlier leader, or by itself
        I.gpos[k] = g;                                // ordinal of the leader (groups_kernel's sort key; it overwrites gpos afterwards)
        const float* m = overlap_src<SRC>(src, I, b, N, ld);
        I.plead[k] = overlap_at<SRC>(m, ld, I.order[k], I.leadc[g], thr);    // likewise overwritten by groups_kernel's own plead
    }
}

// K4 for one image by its WHOLE workgroup (1024 threads; the chain kernels below).  sym: the scan has attributed (rem[] final); what
// is left per rank is three levels of dependent gathers (leader ordinal, order / leadc, the two boxes) whose latency beside the write
// stream is microseconds each: four ranks of a thread side by side, every load of a level issued before the first use, stores last.
template <int SRC>
__device__ __forceinline__ void attribute_image(const float* __restrict__ src, long ld, int N, const int* __restrict__ counts, float thr, char* ws,
                                                gnms_ws_layout L, const int b, const int sym_arg) {
    const int tid = threadIdx.x;
    const int sym = sym_arg == 2 ? (img_ptrs(ws, L, b).misc[3] == 0 ? 1 : 0) : sym_arg;
    if (!sym) {
        for (int kb = tid >> 6; kb < L.NB; kb += 16) attribute_body<SRC>(src, ld, N, counts, thr, ws, L, b, kb, tid & 63, 0);
        return;
    }
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float* m = overlap_src<SRC>(src, I, b, N, ld);
    for (int k0 = 0; k0 < n; k0 += 4096) {
        int g4[4], ca[4], cb[4], lr4[4];
        float pl[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + tid + e * 1024;
            const bool ok = k < n;
            lr4[e] = ok ? rem_load(I.rem, k) : 0;
            ca[e] = ok ? I.order[k] : 0;
        }
        // (the leader's input index is order[its rank]: the same value as leadc[its ordinal], one dependent load earlier)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int lr = lr4[e];
            g4[e] = I.leadpfx[lr >> 6] + __builtin_popcountll(I.leadw[lr >> 6] & ((1ull << (lr & 63)) - 1ull));
            cb[e] = (k0 + tid + e * 1024 < n) ? I.order[lr] : 0;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) pl[e] = (k0 + tid + e * 1024 < n) ? overlap_at<SRC>(m, ld, ca[e], cb[e], thr) : 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + tid + e * 1024;
            if (k < n) { I.gpos[k] = g4[e]; I.plead[k] = pl[e]; }
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(64) void attribute_kernel(const float* __restrict__ src, long ld, int N, const int* __restrict__ counts, float thr,
                                                       char* ws, gnms_ws_layout L, int sym) {
    attribute_body<SRC>(src, ld, N, counts, thr, ws, L, (int)blockIdx.y, (int)blockIdx.x, (int)threadIdx.x, sym);
}

// ------------------------------------------------------------------------------------------------
// K5: groups.  member(k) = iou[order[k]][order[rem[k]]] > thr (strict, :249); sort (leader, rank) in LDS;
// runs of equal leader are the groups, their first group_size+1 entries survive (:253-255), the first
// entry is the column the mask keeps (:99).  MASKED: the default rescoring (:95-105,:111) is fused:
//   pre_k = s_k - prune(iou[k][head]) * s_head      (I - P restricted to the head column)
// Arrays head/gpos/gstart/glen/gsorted/plead are indexed by rank; pre is indexed by NMS position q
// (q = rank for hard sort, q = input index when presorted).
// ------------------------------------------------------------------------------------------------
// FUSE (E <= 4, the chain kernels after a scan that has attributed: leaders_body with sym): K4's work -- the leader's ordinal and the
// overlap with it -- is done HERE, for the very ranks phase 1 and phase 3 of this thread own (k = e * 1024 + t), and what K4 would have
// parked in global memory for them (gpos, plead) or they would have loaded again (order, sscore, rem, the leader's score) stays in
// registers across the sort.  Beside the matrix writers every dependent global load of the chain costs ~2 us: K4 -> barrier -> K5 was
// eight levels of them, this is four (rem / order / sscore -> the leader's order, score, ordinal -> the two boxes -> stores).
constexpr int kBigGroupList = 16;     // groups above this size are also listed from the end of hlist (groups_body, solve_groups_kernel)

// ------------------------------------------------------------------------------------------------
// The BACKWARD PLAN (masked groups, scores not pre-sorted): what bwd_plan_kernel needs to know about position p, in one 8-byte entry, so
// that the backward is "entry -> pre / plead / dL/dprob -> store" and nothing of head / glen / hlist / gstart / gsorted / order / misc is
// on its path.  Positions follow the runs of gsorted: [0, total) the members run after run in rank order, [total, n) the ranks in no
// group (and, inside a run K5 proper cut at the cap, the candidates cut off: same role), [n, N) padding.
//   low word : rank mk (14 bits) | input index order[mk] << 14 (where dL/ds goes)
//   high word: offset inside the run (14 bits) | run length << 14 (15 bits; on the run's first entry; <= N <= 16384) | role << 29 | padding << 31
// Every builder of the runs writes it through plan_entry / plan_pad (or, where one thread knows the rank and another the run's length, the
// two words separately: plan_lo / plan_hi), every call: the plan is never older than the runs beside it.
// ------------------------------------------------------------------------------------------------
constexpr int kPlanHalo = 128;              // members behind a head that bwd_plan_kernel sums from its tile of products (the default cap is 100 + 1)
constexpr unsigned kPlanZero = 0u;          // in no group: dL/ds = 0
constexpr unsigned kPlanMember = 1u;        // a member (or the head of a group of one): dL/ds = gx
constexpr unsigned kPlanHead = 2u;          // head of a run of 2 .. kPlanHalo + 1 members: gx - sum of the following entries' products
constexpr unsigned kPlanLongHead = 3u;      // head of a longer run: a whole wave walks the run
constexpr unsigned kPlanPadBit = 1u << 31;  // (high word) position >= n: dL/ds[p] = 0, gx[p] = 0
__device__ __forceinline__ unsigned plan_lo(int mk, int dst) { return (unsigned)mk | ((unsigned)dst << 14); }
// rank `off` places behind the head of a run of `len` members (len counts on the head only); member = false: in no group
__device__ __forceinline__ unsigned plan_hi(int off, int len, bool member) {
    const unsigned role = !member ? kPlanZero : ((off != 0 || len <= 1) ? kPlanMember : (len <= kPlanHalo + 1 ? kPlanHead : kPlanLongHead));
    return ((unsigned)off & 0x3fffu) | ((off == 0 && member ? (unsigned)len : 0u) << 14) | (role << 29);
}
__device__ __forceinline__ unsigned* plan_word(const ImgPtrs& I, int p, int hi) { return reinterpret_cast<unsigned*>(I.plan + p) + hi; }
// (order through agent-scope loads: in the one launch the sort is a workgroup of the same launch)
__device__ __forceinline__ int plan_dst(const ImgPtrs& I, int mk) { return coh_load(I.order + mk); }
__device__ __forceinline__ void plan_entry(const ImgPtrs& I, int p, int mk, int dst, int off, int len, bool member) {
    I.plan[p] = ((u64)plan_hi(off, len, member) << 32) | plan_lo(mk, dst);
}
// K5's sort key of a rank in no group: the leader bits all ones (no ordinal reaches them), the rank kept below them for the plan;
// padding ranks (k >= n) sort behind them (the sort is stable)
__device__ __forceinline__ unsigned key_no_group(int k, int n) { return k < n ? (0xffffc000u | (unsigned)k) : ~0u; }
__device__ __forceinline__ bool key_is_no_group(unsigned key) { return (key >> 14) == 0x3ffffu; }
__device__ __forceinline__ void plan_pad(const ImgPtrs& I, int p) { I.plan[p] = ((u64)kPlanPadBit << 32) | plan_lo(p, p); }

template <int E, int SRC, bool FUSE = false>
__device__ __forceinline__ void groups_body(const float* __restrict__ iou, int N, long ld, const int* __restrict__ counts,
                                            gnms_params P, char* ws, gnms_ws_layout L, int Ppow2, const int b) {
    static_assert(!FUSE || E <= 4, "the fused attribution keeps five values per owned rank in registers");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem);          // (leader ordinal << 14) | rank : 28 bits (N <= 16384)
    unsigned* info = keys + Ppow2;                               // per rank: head | pos << 14, or ~0 (in no group)
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float* m = overlap_src<SRC>(iou, I, b, N, ld);                      // kFromBoxes: `iou` holds the boxes [B][N][4]
    const float thr = P.nms_threshold;
    // ---- phase 1: membership key of every rank, lane-contiguous ranks (k = e * blockDim + t: coalesced loads), straight into LDS ----
    GNMS_T0();
    // key = (ordinal of the leader << 14) | rank: the ordinal (attribute_kernel left it in gpos, with the overlap against that
    // leader in plead) needs only log2(#leaders) bits, i.e. ONE 7-bit radix pass for up to 127 groups
    int f_lr[FUSE ? E : 1], f_ck[FUSE ? E : 1];                       // FUSE: rem[k], order[k], sscore[k], overlap with and score of the leader
    float f_sk[FUSE ? E : 1], f_pl[FUSE ? E : 1], f_sl[FUSE ? E : 1];
    if constexpr (FUSE) {
        int g[E], cb[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * (int)blockDim.x + (int)threadIdx.x;
            const bool ok = k < n;
            f_lr[e] = ok ? rem_load(I.rem, k) : 0;
            f_ck[e] = ok ? I.order[k] : 0;
            f_sk[e] = ok ? I.sscore[k] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int lr = f_lr[e];
            g[e] = I.leadpfx[lr >> 6] + __builtin_popcountll(I.leadw[lr >> 6] & ((1ull << (lr & 63)) - 1ull));
            cb[e] = I.order[lr];                                        // (= leadc[g]: the leader's input index)
            f_sl[e] = I.sscore[lr];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * (int)blockDim.x + (int)threadIdx.x;
            f_pl[e] = (k < n) ? overlap_at<SRC>(m, ld, f_ck[e], cb[e], thr) : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * (int)blockDim.x + (int)threadIdx.x;
            keys[k] = (k < n && f_pl[e] > thr) ? (((unsigned)g[e] << 14) | (unsigned)k) : key_no_group(k, n);   // strict > (:249)
            info[k] = ~0u;
        }
    } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * (int)blockDim.x + (int)threadIdx.x;
        unsigned key = key_no_group(k, n);
        if (k < n && I.plead[k] > thr) key = ((unsigned)I.gpos[k] << 14) | (unsigned)k;     // strict > (:249)
        keys[k] = key;
        info[k] = ~0u;
    }
    }
    GNMS_TACC(8);
    // group by leader: the keys start in rank order, so a STABLE sort on the leader bits alone yields (leader, rank) order
    __shared__ unsigned radix_hist[128 * 16 + 16];
    __syncthreads();
    {
        const int G = I.misc[0];                                           // number of leaders; the all-ones digit is reserved for the padding keys
        block_radix_pass7<E>(keys, 14, radix_hist);
        if (G > 127) block_radix_pass7<E>(keys, 21, radix_hist);
        if (G > 16383) block_radix_pass7<E>(keys, 28, radix_hist);
    }
    GNMS_TACC(9);
    // ---- phase 2: runs of equal leader are the groups; cap, head, position.  Thread t owns sorted positions
    //      t*E .. t*E+E-1; the start of each position's run comes from a max-scan of the run-start flags
    //      (registers -> wave shuffles -> 16 per-wave totals in LDS): no per-element search. ----
    const long long cap = (long long)P.group_size + 1;
    const bool plan = P.mask_group_boxes && !P.presorted;             // the backward plan: for the route that reads it (bwd_plan_kernel)
    __shared__ int wave_last_start[16];
    {
        const int t = threadIdx.x, ln = t & 63, wv = t >> 6;
        unsigned ky[E];
        int st[E];                                                     // run start of position i, or -1 if it lies in an earlier thread
        int last = -1;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = t * E + e;
            ky[e] = keys[i];
            const bool valid = !key_is_no_group(ky[e]);
            const bool first = valid && (i == 0 || (keys[i - 1] >> 14) != (ky[e] >> 14));
            if (first) last = i;
            st[e] = last;
        }
        // inclusive max-scan of `last` over the wave, then exclusive value for this thread
        const int inc = gnms_max_scan32(last);                         // DPP running maximum
        int excl = __builtin_amdgcn_update_dpp(-1, inc, 0x138, 0xF, 0xF, false);   // wave_shr:1 (lane 0 keeps -1)
        if (ln == 0) excl = -1;
        if (ln == 63) wave_last_start[wv] = inc;
        __syncthreads();
        int carry = -1;
        for (int w = 0; w < wv; ++w) carry = max(carry, wave_last_start[w]);
        const int before = max(excl, carry);
        // the plan (see plan_entry): this thread knows which rank sits at its positions -> the low words, all gathers of order[] in one
        // batch; the high word of a run's first entry comes from the thread that sees the run end
        if (plan) {
            int pdst[E];
#pragma unroll
            for (int e = 0; e < E; ++e) pdst[e] = (t * E + e < n) ? plan_dst(I, (int)(ky[e] & 0x3fffu)) : 0;
#pragma unroll
            for (int e = 0; e < E; ++e) if (t * E + e < n) *plan_word(I, t * E + e, 0) = plan_lo((int)(ky[e] & 0x3fffu), pdst[e]);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = t * E + e;
            bool big_head = false;
            int hk = 0;
            if (i < n) {
                if (!key_is_no_group(ky[e])) {
                    const int k = (int)(ky[e] & 0x3fffu);
                    const int start = st[e] >= 0 ? st[e] : before;
                    const long long pos = i - start;
                    const unsigned hd = keys[start] & 0x3fffu;
                    if (pos < cap) info[k] = hd | ((unsigned)pos << 14);
                    if (plan && pos > 0) *plan_word(I, i, 1) = plan_hi((int)pos, 0, pos < cap);
                    const bool lastofrun = (i + 1 >= n) || key_is_no_group(keys[i + 1]) || ((keys[i + 1] >> 14) != (ky[e] >> 14));
                    if (lastofrun) {                                  // the run's last element publishes the extent for the head
                        const long long len = pos + 1;
                        I.gstart[hd] = start;
                        I.glen[hd] = (int)(len < cap ? len : cap);
                        if (plan) *plan_word(I, start, 1) = plan_hi(0, (int)(len < cap ? len : cap), true);
                        big_head = len > 1;
                        hk = (int)hd;
                        // groups of more than kBigGroupList members are listed a second time, from the END of hlist (misc[4] of them): the
                        // unmasked solves hand those to whole workgroups and everything smaller to single waves (nms_solve_kernels.h)
                        if ((len < cap ? len : cap) > kBigGroupList) I.hlist[N - 1 - atomicAdd(&I.misc[4], 1)] = hk;
                    }
                } else if (plan) {
                    *plan_word(I, i, 1) = plan_hi(0, 0, false);                      // in no group: the stable sort kept these in rank order behind the runs
                }
            }
            // heads of multi-member groups go to hlist (one atomic per wave)
            const unsigned long long bm = __ballot(big_head);
            if (bm) {
                int base = 0;
                if (ln == __builtin_ctzll(bm)) base = atomicAdd(&I.misc[1], __builtin_popcountll(bm));
                base = __builtin_amdgcn_readlane(base, __builtin_ctzll(bm));
                if (big_head) I.hlist[base + __builtin_popcountll(bm & ((1ull << ln) - 1ull))] = hk;
            }
        }
    }
    // members in (group, rank) order, written lane-contiguously straight from the sorted keys
    if (plan) for (int i = n + (int)threadIdx.x; i < N; i += blockDim.x) plan_pad(I, i);
    for (int i = threadIdx.x; i < n; i += blockDim.x) I.gsorted[i] = key_is_no_group(keys[i]) ? -1 : (int)(keys[i] & 0x3fffu);
    __syncthreads();
    GNMS_TACC(10);
    // ---- phase 3 (lane-contiguous ranks k = e * blockDim + t: every load and store below is coalesced; with the thread-contiguous
    //      ownership of phase 1 the stores of a wave were E * 4 bytes apart -- a different 64-byte line per lane at E = 16):
    //      group fields and, for MASKED groups, the default rescoring
    //      pre_k = s_k - prune(iou[k][head]) * s_head  (I - P restricted to the head column, :95-105,:111) ----
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * (int)blockDim.x + (int)threadIdx.x;
        if (k >= N) continue;
        const unsigned inf = info[k];
        const int h = (k < n && inf != ~0u) ? (int)(inf & 0x3fffu) : -1;
        I.head[k] = h;
        I.gpos[k] = (h >= 0) ? (int)(inf >> 14) : -1;
        if (h != k) I.glen[k] = 0;                                   // only heads carry an extent
        if (!P.mask_group_boxes) continue;
        float pre = 0.0f, pl = 0.0f;
        int ck;
        float sk;
        if constexpr (FUSE) { ck = f_ck[e]; sk = f_sk[e]; }
        else { ck = (k < n) ? I.order[k] : 0; sk = (k < n) ? I.sscore[k] : 0.0f; }
        const int q = P.presorted ? ck : k;
        if (h == k) {
            pre = sk;
        } else if (h >= 0) {
            int lr;
            if constexpr (FUSE) lr = f_lr[e]; else lr = rem_load(I.rem, k);
            float v, sh;
            int ch;
            if (h != lr) {                                           // the leader itself is not a member (NaN / <= thr diagonal)
                ch = I.order[h];
                v = overlap_at<SRC>(m, ld, ck, ch, thr);
                sh = I.sscore[h];
            } else {
                ch = -1;
                if constexpr (FUSE) { v = f_pl[e]; sh = f_sl[e]; }
                else {
                    v = I.plead[k];                                  // overlap with the leader, left there by attribute_kernel
                    sh = I.sscore[lr];
                }
            }
            bool tril = true;                                        // torch.tril in NMS order (:72): always true for hard sort
            if (P.presorted) { if (ch < 0) ch = I.order[h]; tril = ch < ck; }
            if (tril) pl = gnms_prune(v, thr, P.temperature, P.pruning_method);
            pre = sk - pl * sh;
        }
        I.plead[k] = pl;
        I.pre[(k < n) ? q : k] = pre;
        if constexpr (FUSE) {
            // K6 starts from the clamped value by NMS position and ends with the input indices of the listed boxes: both are at hand
            // here and wait for it in LDS (beyond keys / info, both dead for this thread's rank by now) -- finalize_body<E, true> then
            // begins without a global load and the barrier in front of it need not wait for the stores above
            if (k < n) {
                const float r2 = pre < 0.0f ? 0.0f : (pre > 1.0f ? 1.0f : pre);      // torch.clamp keeps NaN
                I.r2[q] = r2;
                reinterpret_cast<float*>(smem)[q] = r2;                              // finalize_body's `stage` (the key region)
                reinterpret_cast<int*>(smem + (size_t)Ppow2 * 8)[k] = ck;            // order[] by rank
                reinterpret_cast<float*>(smem + (size_t)Ppow2 * 12)[q] = r2;         // a copy the key sort does not overwrite
            }
        }
    }
    GNMS_TACC(11);
}

template <int E, int SRC>
__global__ __launch_bounds__(1024) void groups_kernel(const float* __restrict__ iou, int N, long ld, const int* __restrict__ counts,
                                                      gnms_params P, char* ws, gnms_ws_layout L, int Ppow2) {
    groups_body<E, SRC>(iou, N, ld, counts, P, ws, L, Ppow2, (int)blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// K6: finalize (lib/groomed_nms.py:111-129).  r2 = clamp(pre,0,1); r = r2 with (< valid_thr) zeroed;
// the reference then sorts r descending (:116-121).  After thresholding every invalid box is an exact 0,
// so a STABLE descending sort is: [NaN boxes by position][valid boxes by (r desc, position)][invalid boxes
// by position].  Only the valid subset needs a sort; the other two are stream compactions (one packed
// block scan).  valid / invalid are INPUT indices padded with -1; prob is written in the order the
// reference returns it.
// ------------------------------------------------------------------------------------------------
// STAGED (behind groups_body<E, SRC, true>, masked groups): the clamped values already sit in `stage` and the input index of every
// rank in LDS behind the key region (ordL); r2 is in global memory as well.
template <int E, bool STAGED = false>
__device__ __forceinline__ void finalize_body(int N, const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                              int Ppow2, float* __restrict__ prob, long long* __restrict__ valid,
                                              long long* __restrict__ invalid, int* __restrict__ nvalid, int* __restrict__ ninvalid,
                                              const int b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                     // [Ppow2]
    __shared__ u64 wave_tot[16];
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float vthr = P.valid_box_prob_threshold;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, T = blockDim.x;
    GNMS_T0();
    // clamp: global loads and stores with lane-contiguous positions (coalesced), staged in LDS for the owner threads below,
    // which need thread-contiguous positions so that the compaction keeps the order
    float* stage = reinterpret_cast<float*>(smem);                 // [Ppow2] floats inside the key region (not yet in use)
    const int* ordL = reinterpret_cast<const int*>(smem + (size_t)Ppow2 * 8);   // STAGED: order[] by rank, behind the key region
    if constexpr (!STAGED) {
        for (int q = t; q < n; q += T) {
            const float pre = I.pre[q];
            const float r2 = pre < 0.0f ? 0.0f : (pre > 1.0f ? 1.0f : pre);          // torch.clamp keeps NaN
            I.r2[q] = r2;
            stage[q] = r2;
        }
        __syncthreads();
    }
    // classify
    u64 key[E];
    int cls[E];                                                    // 0 nan, 1 valid, 2 invalid, 3 padding
    u64 packed = 0;                                                // nan | valid << 16 | invalid << 32 (each count <= N <= 16384)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int q = t * E + e;
        cls[e] = 3;
        key[e] = ~0ull;
        if (q < n) {
            const float r2 = stage[q];
            const float rr = (r2 < vthr) ? 0.0f : r2;                           // :115
            cls[e] = (rr != rr) ? 0 : ((rr >= vthr) ? 1 : ((rr < vthr) ? 2 : 0)); // vthr NaN: neither list (:118-123)
            key[e] = ((u64)gnms_desc_key(rr) << 32) | (unsigned)q;
            packed += (cls[e] == 0) ? 1ull : (cls[e] == 1 ? (1ull << 16) : (1ull << 32));
        }
    }
    // exclusive block scan of the packed counters
    // (two 32-bit DPP prefix sums: the low word carries nan | valid << 16 without overflow between the fields, the high word invalid)
    const u64 inc = (u64)gnms_add_scan32((unsigned)(packed & 0xffffffffu)) | ((u64)gnms_add_scan32((unsigned)(packed >> 32)) << 32);
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();                                               // every owner has read its staged values
    u64 base = 0, total = 0;
    const int nwaves = T >> 6;
    for (int w = 0; w < nwaves; ++w) { const u64 v = wave_tot[w]; if (w < wave) base += v; total += v; }
    u64 run = base + inc - packed;
    const int n_nan = (int)(total & 0xffff), nv = (int)((total >> 16) & 0xffff), ni = (int)(total >> 32);
    const int n_ge = n_nan + nv;
    if (!valid && !invalid && !P.return_sorted_prob) {
        // the caller wants the probabilities only (training reads just the third return value, lib/loss/rpn_3d.py:791):
        // no compaction, no sort of the valid boxes -- only the counts and prob
        float* pbq = prob + (size_t)b * N;
        for (int j = t; j < N; j += T) {
            float out = 0.0f;
            // (STAGED: no full barrier since groups_body stored r2 -- the staged copy is the one every thread can see)
            if (j < n) { const float r2j = STAGED ? stage[j] : I.r2[j]; out = P.group_boxes ? r2j : ((r2j < vthr) ? 0.0f : r2j); }   // :124-127
            pbq[j] = out;
            I.sidx[j] = j;
        }
        if (t == 0) {
            if (nvalid) nvalid[b] = nv;
            if (ninvalid) ninvalid[b] = ni;
        }
        return;
    }
    for (int i = t; i < Ppow2; i += T) keys[i] = ~0ull;           // (the staged values end here)
    __syncthreads();
    // sidx layout: [0,n_nan) NaN by position, [n_nan, n_ge) valid (sorted below), [n_ge, n_ge+ni) invalid by position
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int q = t * E + e;
        if (cls[e] == 0) { I.sidx[(int)(run & 0xffff)] = q; run += 1ull; }
        else if (cls[e] == 1) { keys[(int)((run >> 16) & 0xffff)] = key[e]; run += 1ull << 16; }
        else if (cls[e] == 2) {
            const int j = (int)(run >> 32);
            I.sidx[n_ge + j] = q;
            if (invalid) invalid[(size_t)b * N + j] = P.presorted ? q : (STAGED ? ordL[q] : I.order[q]);
            run += 1ull << 32;
        }
    }
    __syncthreads();
    GNMS_TACC(12);
    // sort the valid keys: they sit in keys[0..nv), padded with ~0
    if (nv > 1) {
        if (nv <= 256 && 2 * nv <= Ppow2) {
            // a few valid boxes (typically ~100): rank of each key = number of smaller keys (they are distinct), read as LDS broadcasts
            u64* sorted = keys + Ppow2 / 2;
            u64 mine = 0;
            int rank = 0;
            if (t < nv) {
                mine = keys[t];
                for (int j = 0; j < nv; ++j) rank += (keys[j] < mine) ? 1 : 0;
            }
            __syncthreads();
            if (t < nv) sorted[rank] = mine;
            __syncthreads();
            if (t < nv) keys[t] = sorted[t];
            __syncthreads();
        } else if (nv <= T) {
            u64 r1[1] = {keys[t]};
            __syncthreads();
            int pe = 64;                                                   // typically ~100 valid boxes: 128 keys, one merge pass instead of four
            while (pe < nv) pe <<= 1;
            block_sort<1, u64>(r1, keys, pe);
        } else {
            // more valid boxes than threads: sort next_pow2(nv) keys, not all Ppow2 (the valid keys are compacted at the front)
            int pe = 2 * T;
            while (pe < nv) pe <<= 1;
            bool done = false;
            if constexpr (E >= 4) {
                if (pe == 2 * T) {
                    u64 r[2];
                    r[0] = keys[t * 2]; r[1] = keys[t * 2 + 1];
                    __syncthreads();
                    block_sort<2, u64>(r, keys, pe);
                    done = true;
                }
            }
            if constexpr (E >= 8) {
                if (!done && pe == 4 * T) {
                    u64 r[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = keys[t * 4 + e];
                    __syncthreads();
                    block_sort<4, u64>(r, keys, pe);
                    done = true;
                }
            }
            if constexpr (E >= 16) {
                if (!done && pe == 8 * T) {
                    u64 r[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) r[e] = keys[t * 8 + e];
                    __syncthreads();
                    block_sort<8, u64>(r, keys, pe);
                    done = true;
                }
            }
            if (!done) {
                u64 r[E];
#pragma unroll
                for (int e = 0; e < E; ++e) r[e] = keys[t * E + e];
                __syncthreads();
                block_sort<E, u64>(r, keys, Ppow2);
            }
        }
    }
    GNMS_TACC(13);
    float* pb = prob + (size_t)b * N;
    for (int j = t; j < N; j += T) {
        if (j < nv) {
            const int q = (int)(keys[j] & 0xffffffffu);
            I.sidx[n_nan + j] = q;
            if (valid) valid[(size_t)b * N + j] = P.presorted ? q : (STAGED ? ordL[q] : I.order[q]);
        } else if (valid) valid[(size_t)b * N + j] = -1;
        if (j >= ni && invalid) invalid[(size_t)b * N + j] = -1;
        if (j >= n) I.sidx[j] = j;
    }
    // (STAGED, unsorted output: every value of the last loop comes from LDS -- no barrier for sidx, no global load)
    const float* r2L = reinterpret_cast<const float*>(smem + (size_t)Ppow2 * 12);
    if (!STAGED || P.return_sorted_prob) __syncthreads();
    for (int j = t; j < N; j += T) {
        float out = 0.0f;
        if (j < n) {
            if (P.return_sorted_prob) { const int sj = I.sidx[j]; const float r2q = STAGED ? r2L[sj] : I.r2[sj]; out = (r2q < vthr) ? 0.0f : r2q; }   // :117
            else { const float r2j = STAGED ? r2L[j] : I.r2[j]; out = P.group_boxes ? r2j : ((r2j < vthr) ? 0.0f : r2j); }       // :124-127
        }
        pb[j] = out;
    }
    GNMS_TACC(14);
    if (t == 0) {
        if (nvalid) nvalid[b] = nv;
        if (ninvalid) ninvalid[b] = ni;
    }
}

template <int E>
__global__ __launch_bounds__(1024) void finalize_kernel(int N, const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                                        int Ppow2, float* __restrict__ prob, long long* __restrict__ valid,
                                                        long long* __restrict__ invalid, int* __restrict__ nvalid,
                                                        int* __restrict__ ninvalid) {
    finalize_body<E>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, (int)blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// The FAST TAIL (round 5): masked groups, hard sort, symmetric scan, N <= 4096.
//   leaders_sb_body<STAGE>   every scan workgroup: head / plead / pre / r2 of its own ranks right behind its resolve (see there)
//   fast_final_body          the image's last scan workgroup: verdict (no leader outside its own group, no group above the cap), then K6
//                            from LDS -- or, verdict "slow", K5 proper (groups_body) as before
//   csr_build_body           ONE MORE workgroup per image, beside K6: the groups as contiguous runs (gsorted / gstart / glen / gpos / hlist),
//                            which only the backward reads -- a counting sort on the leader's RANK (LDS atomics), members ranked inside
//                            their run by comparison, so that the result does not depend on the order the atomics were served in
// What it takes off the path to the probabilities: the attribution gathers (four dependent levels on one CU -> one level on nsb CUs),
// both radix passes, the run scan and K5's stores: scan + groups + finalize 63 -> ~40 us at B = 8, N = 4096 (profiles/r05*).
// ------------------------------------------------------------------------------------------------
// dynamic LDS: the scan's structures, then cnt[N] (fast_final_body); csr_build_body: 4 arrays of Ppow2 ints
__host__ __device__ __forceinline__ size_t fast_tail_cnt_offset(int NB) { return (leaders_lds_size(NB) + 15) & ~(size_t)15; }
__host__ __device__ __forceinline__ size_t fast_tail_lds_size(int N, int Ppow2) {
    const size_t a = fast_tail_cnt_offset((N + 63) / 64) + (size_t)N * 4, c = (size_t)Ppow2 * 32;     // (finalize_fast_body: 3 arrays + 2 key lists + the bucket segments)
    return a > c ? a : c;
}

// K6 of the fast tail.  In: r2 / head / input index by rank in LDS (fast_final_body).  Same outputs as finalize_body, bit for bit; what
// differs is how the valid boxes get into descending order.  A valid HEAD carries r = clamp(its own score), and the ranks ARE the scores in
// descending order (clamp is monotone, ties keep their positions): the valid heads, compacted in rank order, are a sorted run as they
// stand (list A; checked, one compare per element -- a violation sends everything through the sort).  Only the other valid boxes (members
// whose rescored value stayed above the threshold: list B, typically a few dozen) are sorted, and the two lists are merged by rank
// (position in the own list + binary search in the other).  For ~1 900 valid boxes of 4 096 that replaces a 2 048-key merge sort (9 us on
// one CU) by a compaction, a small sort and 11 LDS probes per box.  No global load and no wait for a global store anywhere.
constexpr int kDirectMergeMax = 256;     // boxes of list B up to which K6 of the fast tail places them by counting (finalize_fast_body)
template <int E>
__device__ __forceinline__ void finalize_fast_body(int N, const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                                   int Ppow2, float* __restrict__ prob, long long* __restrict__ valid,
                                                   long long* __restrict__ invalid, int* __restrict__ nvalid, int* __restrict__ ninvalid,
                                                   const int b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float* r2L = reinterpret_cast<const float*>(smem);
    const int* hdL = reinterpret_cast<const int*>(smem + (size_t)Ppow2 * 4);
    const int* ordL = reinterpret_cast<const int*>(smem + (size_t)Ppow2 * 8);
    u64* keyA = reinterpret_cast<u64*>(smem + (size_t)Ppow2 * 12);                   // [Ppow2] valid heads, in rank order
    u64* keyB = reinterpret_cast<u64*>(smem + (size_t)Ppow2 * 20);                   // [Ppow2] the other valid boxes
    __shared__ unsigned ff_tot[2][16];
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float vthr = P.valid_box_prob_threshold;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float* pb = prob + (size_t)b * N;
    GNMS_T0();
    // classify, thread-contiguous positions (the compaction keeps the order)
    u64 key[E];
    int cls[E];                                                    // 0 nan, 1 valid head, 2 valid other, 3 invalid, 4 padding
    unsigned w0 = 0u, w1 = 0u;                                     // nan | heads << 16,  others | invalid << 16  (each count <= 4096)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int q = t * E + e;
        cls[e] = 4;
        key[e] = ~0ull;
        if (q < n) {
            const float r2 = r2L[q];
            const float rr = (r2 < vthr) ? 0.0f : r2;                              // :115
            cls[e] = (rr != rr) ? 0 : ((rr >= vthr) ? (hdL[q] == q ? 1 : 2) : ((rr < vthr) ? 3 : 0));   // vthr NaN: neither list (:118-123)
            key[e] = ((u64)gnms_desc_key(rr) << 32) | (unsigned)q;
            w0 += (cls[e] == 0) ? 1u : (cls[e] == 1 ? (1u << 16) : 0u);
            w1 += (cls[e] == 2) ? 1u : (cls[e] == 3 ? (1u << 16) : 0u);
        }
    }
    const unsigned inc0 = gnms_add_scan32(w0), inc1 = gnms_add_scan32(w1);
    if (lane == 63) { ff_tot[0][wave] = inc0; ff_tot[1][wave] = inc1; }
    lds_barrier();
    unsigned base0 = 0u, base1 = 0u, tot0 = 0u, tot1 = 0u;
    for (int w = 0; w < 16; ++w) {
        const unsigned a = ff_tot[0][w], c = ff_tot[1][w];
        if (w < wave) { base0 += a; base1 += c; }
        tot0 += a; tot1 += c;
    }
    const int n_nan = (int)(tot0 & 0xffffu), ni = (int)(tot1 >> 16);
    int nA = (int)(tot0 >> 16), nB = (int)(tot1 & 0xffffu);
    const int nv = nA + nB, n_ge = n_nan + nv;
    // the two counts leave as soon as they are known: where they go to pinned host memory (gnms_host_counts_slot: the reference's index
    // tensors have a data-dependent length) the host takes them ~3 us before the lists below are complete -- which it does not read; whatever
    // it enqueues next is behind this launch on the stream
    if (t == 0) { if (nvalid) nvalid[b] = nv; if (ninvalid) ninvalid[b] = ni; }
    if (!valid && !invalid && !P.return_sorted_prob) {
        // the caller wants the probabilities only (training reads just the third return value, lib/loss/rpn_3d.py:791)
        for (int j = t; j < N; j += 1024) pb[j] = (j < n) ? r2L[j] : 0.0f;                    // (grouped mode: the un-thresholded clone, :124-125)
        return;
    }
    const bool sorted_out = P.return_sorted_prob != 0;
    // (the bucket counters of the merge below live where the heads were: every thread has read its heads in front of the barrier above)
    for (int i = t; i < Ppow2; i += 1024) reinterpret_cast<int*>(smem + (size_t)Ppow2 * 4)[i] = 0;
    // compaction.  sidx layout: [0, n_nan) NaN by position, [n_nan, n_ge) valid (merged below), [n_ge, n_ge + ni) invalid by position
    // (sidx is the backward's map for the SORTED output only, bwd_gx_kernel: written only then)
    {
        unsigned run0 = base0 + inc0 - w0, run1 = base1 + inc1 - w1;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int q = t * E + e;
            if (cls[e] == 0) { const int p = (int)(run0 & 0xffffu); if (sorted_out) { I.sidx[p] = q; pb[p] = r2L[q]; } run0 += 1u; }
            else if (cls[e] == 1) { keyA[run0 >> 16] = key[e]; run0 += 1u << 16; }
            else if (cls[e] == 2) { keyB[run1 & 0xffffu] = key[e]; run1 += 1u; }
            else if (cls[e] == 3) {
                const int j = (int)(run1 >> 16);
                if (invalid) invalid[(size_t)b * N + j] = ordL[q];
                if (sorted_out) { I.sidx[n_ge + j] = q; pb[n_ge + j] = 0.0f; }     // (thresholded, :115-117)
                run1 += 1u << 16;
            }
        }
    }
    lds_barrier();
    GNMS_TACC(12);
    // the heads must be a sorted run (they are, whenever the scores were finite and the ranks their descending order)
    int viol = 0;
    for (int i = t + 1; i < nA; i += 1024) viol |= keyA[i] <= keyA[i - 1];
    if (t < kDirectMergeMax) reinterpret_cast<int*>(smem + (size_t)Ppow2 * 28)[t] = 0;      // (the counting merge's ranks; nobody else is in that region yet)
    viol = __syncthreads_or(viol);
    auto emit = [&](const u64 k, const int p) {
        const int q = (int)(k & 0xffffffffu);
        if (valid) valid[(size_t)b * N + p] = ordL[q];
        if (sorted_out) { I.sidx[n_nan + p] = q; pb[n_nan + p] = r2L[q]; }   // (valid: >= the threshold, returned as it is)
    };
    if (viol) {                                                    // never seen; kept exact: everything through the sort
        for (int i = t; i < nA; i += 1024) keyB[nB + i] = keyA[i];
        nB += nA;
        u64 r[E];
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] = (t * E + e < nB) ? keyB[t * E + e] : ~0ull;
        lds_barrier();
        block_sort<E, u64>(r, keyB, E * 1024);
        for (int i = t; i < nB; i += 1024) emit(keyB[i], i);
    } else if (nB == 0) {
        for (int i = t; i < nA; i += 1024) emit(keyA[i], i);
    } else if (nB <= kDirectMergeMax) {
        // FEW other valid boxes (up to 256; ~100-200 of 4 096 uniform boxes): no bucket counters, no prefix over the heads, no scatter by
        // atomics.  A box of B ends up at (heads in front of it: a binary search) + (boxes of B in front of it: its rank in B, counted --
        // nB^2 compares spread over all 1024 threads, thread (box, segment), the reads of a wave at ONE LDS address); the bucket numbers g
        // laid out by that rank are a sorted list, and head i ends up at i + (boxes of B whose bucket is <= i: a binary search in it).
        // Two barriers, two binary searches and nB^2 / 1024 compares per thread where the bucket merge has five barriers, two rounds of
        // LDS atomics and a scan.  Same positions -- the keys are distinct, the order is total.
        int* cntB = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 28);             // [kDirectMergeMax] rank of each box of B (zeroed in front of the barrier above)
        int* gS = cntB + kDirectMergeMax;                                          // [nB] bucket numbers in B's sorted order
        {
            int lgP = 6;
            while ((1 << lgP) < nB) ++lgP;                                         // P = 64 .. 256 boxes side by side, S = 1024 / P segments
            const int j = t & ((1 << lgP) - 1), sg = t >> lgP, S = 1024 >> lgP, per = (nB + S - 1) / S;
            const int x0 = sg * per, x1 = min(nB, x0 + per);
            if (j < nB && x0 < x1) {
                const u64 k = keyB[j];
                int c = 0, x = x0;
                for (; x + 4 <= x1; x += 4) c += (keyB[x] < k ? 1 : 0) + (keyB[x + 1] < k ? 1 : 0) + (keyB[x + 2] < k ? 1 : 0) + (keyB[x + 3] < k ? 1 : 0);
                for (; x < x1; ++x) c += keyB[x] < k ? 1 : 0;
                if (c) atomicAdd(&cntB[j], c);
            }
        }
        lds_barrier();
        if (t < nB) {
            const u64 k = keyB[t];
            const int r = cntB[t], g = lower_bound_lds<u64>(keyA, nA, k);
            gS[r] = g;
            emit(k, g + r);
        }
        lds_barrier();
        for (int i = t; i < nA; i += 1024) {
            int lo = 0, hi = nB;                                                   // boxes of B with bucket <= i
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (gS[mid] <= i) lo = mid + 1; else hi = mid; }
            emit(keyA[i], i + lo);
        }
    } else {
        // MERGE BY BUCKETS.  The sorted heads split the key space into nA + 1 buckets; a box of B lies in bucket g = number of heads in front
        // of it (a binary search), and its final position is g + (boxes of B in earlier buckets) + (its rank among its bucket mates); head
        // i ends up at i + (boxes of B in buckets <= i).  So B is not sorted as long as the buckets are small (a box or two on detector-like
        // scores): count per bucket (LDS atomics), prefix over the buckets, members scattered into their bucket's segment (the scatter's
        // atomics turn the exclusive prefix into the inclusive one), rank inside the segment by comparison.  A bucket of more than
        // kBucketMax boxes -- scores that nearly tie put every rescored member behind the last head: the C3 harness's random-init network
        // does exactly that, 2 281 boxes in one bucket, and ranking them by comparison took 0.5 ms -- sends B through the sort instead.
        // (nB >= 1, hence nA + 1 <= n <= Ppow2 counters: the head array, dead by now.)
        constexpr int kBucketMax = 32;
        int* cntG = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 4);              // [nA + 1] (zeroed during the compaction above)
        int* seg = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 28);              // [nB] indices into keyB, bucket by bucket
        int gB[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = t + e * 1024;
            gB[e] = 0;
            if (i < nB) { gB[e] = lower_bound_lds<u64>(keyA, nA, keyB[i]); atomicAdd(&cntG[gB[e]], 1); }
        }
        lds_barrier();
        int big;
        {   // exclusive prefix over the nA + 1 buckets, in place (thread t owns buckets t * E .. t * E + E - 1); the largest bucket on the way
            int c[E], sum = 0, mx = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) { const int g = t * E + e; c[e] = (g <= nA) ? cntG[g] : 0; sum += c[e]; mx = max(mx, c[e]); }
            const unsigned inc = gnms_add_scan32((unsigned)sum);
            if (lane == 63) ff_tot[0][wave] = inc;
            big = __syncthreads_or(mx > kBucketMax);
            unsigned base = 0u;
            for (int w = 0; w < 16; ++w) if (w < wave) base += ff_tot[0][w];
            int run = (int)(base + inc) - sum;
#pragma unroll
            for (int e = 0; e < E; ++e) { const int g = t * E + e; if (g <= nA) cntG[g] = run; run += c[e]; }
        }
        lds_barrier();
        if (!big) {
#pragma unroll
            for (int e = 0; e < E; ++e) { const int i = t + e * 1024; if (i < nB) seg[atomicAdd(&cntG[gB[e]], 1)] = i; }
            lds_barrier();                                         // cntG[g] is now the INCLUSIVE prefix: boxes of B in buckets <= g
            for (int i = t; i < nA; i += 1024) emit(keyA[i], i + cntG[i]);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = t + e * 1024;
                if (i < nB) {
                    const int g = gB[e], s0 = g > 0 ? cntG[g - 1] : 0, s1 = cntG[g];
                    const u64 k = keyB[i];
                    int rank = 0;
                    for (int j = s0; j < s1; ++j) rank += keyB[seg[j]] < k ? 1 : 0;
                    emit(k, g + s0 + rank);
                }
            }
        } else {
            // B through the sort; a head's position still comes from the bucket prefix (cntG[i + 1]: boxes of B in buckets <= i)
            for (int i = t; i < nA; i += 1024) emit(keyA[i], i + cntG[i + 1]);
            if (nB <= 1024) {
                u64 r1[1] = {t < nB ? keyB[t] : ~0ull};
                lds_barrier();
                int pe = 64;
                while (pe < nB) pe <<= 1;
                block_sort<1, u64>(r1, keyB, pe);
            } else {
                u64 r[E];
#pragma unroll
                for (int e = 0; e < E; ++e) r[e] = (t * E + e < nB) ? keyB[t * E + e] : ~0ull;
                lds_barrier();
                block_sort<E, u64>(r, keyB, E * 1024);
            }
            for (int j = t; j < nB; j += 1024) { const u64 k = keyB[j]; emit(k, j + lower_bound_lds<u64>(keyA, nA, k)); }
        }
    }
    GNMS_TACC(13);
    for (int j = t; j < N; j += 1024) {
        if (j >= nv && valid) valid[(size_t)b * N + j] = -1;
        if (j >= ni && invalid) invalid[(size_t)b * N + j] = -1;
        if (sorted_out && j >= n) I.sidx[j] = j;
        if (!sorted_out) pb[j] = (j < n) ? r2L[j] : 0.0f;          // (grouped mode: the un-thresholded clone, :124-125)
        else if (j >= n) pb[j] = 0.0f;
    }
    GNMS_TACC(14);
}

template <int E, int SRC, bool FUSED = false>
__device__ __forceinline__ void fast_final_body(const float* __restrict__ src, int N, long ld, const int* __restrict__ counts, gnms_params P,
                                                char* ws, gnms_ws_layout L, int Ppow2, float* __restrict__ prob, long long* __restrict__ valid,
                                                long long* __restrict__ invalid, int* __restrict__ nvalid, int* __restrict__ ninvalid,
                                                const int b, const int last, const unsigned tag = 0u) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* r2L = reinterpret_cast<float*>(smem);                                     // r2 by rank (= position)
    int* hdL = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 4);                     // head by rank
    int* ordL = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 8);                    // input index by rank
    int* cnt = reinterpret_cast<int*>(smem + fast_tail_cnt_offset(L.NB));            // members per leader rank (dead once the verdict is in)
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int tid = threadIdx.x;
    const int nb = (n + 63) >> 6;
    const int nsb = max(1, (nb + kSB - 1) / kSB);
    const int own0 = (nsb - 1) * kSB * 64;                                           // the parked super-block: [own0, n)
    const u64 epoch = FUSED ? ((u64)tag << 32) : ((u64)(unsigned)I.misc[8] << 32);
    const long long cap = (long long)P.group_size + 1;
    int slow = last == 2;
    GNMS_T0();
    if (!slow) {
        // the other super-blocks' ranks: what their workgroups stored (write-through, in front of their granules)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int k = e * 1024 + tid;
            if (k < own0) {
                const int hd = rem_load(I.head, k);
                const float r2 = __hip_atomic_load(I.r2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int ck = I.order[k];
                r2L[k] = r2; hdL[k] = hd; ordL[k] = ck;
            }
        }
        // (a group above kFastGroupMax members also takes K5 proper: csr_build_body ranks the members of a run by comparison, quadratic in its length)
        const long long lim = cap < kFastGroupMax ? cap : kFastGroupMax;
        if (lim < (long long)n) {                                                    // (else no group can be longer than the limit)
            for (int i = tid; i < n; i += 1024) cnt[i] = 0;
            lds_barrier();
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = e * 1024 + tid;
                const int hd = (k < n) ? hdL[k] : -1;
                if (hd >= 0) atomicAdd(&cnt[hd], 1);
            }
            lds_barrier();
            int over = 0;
            for (int i = tid; i < n; i += 1024) over |= (long long)cnt[i] > lim;
            slow = __syncthreads_or(over);
        }
    }
    // this workgroup's own write-through stores (leaders_sb_body) are acknowledged before the verdict -- csr_build_body's go-ahead -- leaves
    GNMS_TACC(8);
    __builtin_amdgcn_s_waitcnt(0x0f70);                                              // vmcnt(0)
    __syncthreads();
    GNMS_TACC(9);
    if (tid == 0) gran_store(I.gran + (size_t)16 * 32 + kGranVerdict, FUSED ? strong_gran(tag, kSlotVerdict + (slow ? 2u : 1u)) : (epoch | (slow ? 2ull : 1ull)));
    if (slow) {
        size_t oa, ol, oc, op;
        leaders_lds_layout(L.NB, &oa, &ol, &oc, &op);
        leaders_epilogue(I, reinterpret_cast<const u64*>(smem + ol), nb, reinterpret_cast<int*>(smem));
        __syncthreads();
        groups_body<E, SRC, true>(src, N, ld, counts, P, ws, L, Ppow2, b);
        lds_barrier();
        finalize_body<E, true>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
        return;
    }
    finalize_fast_body<E>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
}

template <int E, bool FUSED = false>
__device__ __forceinline__ void csr_build_body(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, const int b, const unsigned tag = 0u) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* cnt = reinterpret_cast<int*>(smem);                                         // members per leader rank
    int* fill = cnt + E * 1024;
    int* seg = fill + E * 1024;                                                      // the runs, members in arrival order
    int* startL = seg + E * 1024;
    int* nogroup = startL + E * 1024;                                                // [64] ranks in no group per 64 ranks (E * 16 of them), then their prefix
                                                                                     // (the dynamic LDS of every launch with a CSR workgroup is fast_tail_lds_size: 8 arrays)
    __shared__ int s_cnt[4];                                                         // [0] verdict, [1] multi-member heads, [2] big heads
    __shared__ int wave_tot[16];
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave == 0) {
        const u64* g = I.gran + (size_t)16 * 32 + kGranVerdict;
        u64 v = gran_load(g);
        int verdict;
        if constexpr (FUSED) {                                                       // (strong granules: the launch zeroed nothing)
            const u64 v1 = strong_gran(tag, kSlotVerdict + 1u), v2 = strong_gran(tag, kSlotVerdict + 2u);
            while (v != v1 && v != v2) { __builtin_amdgcn_s_sleep(8); v = gran_load(g); }
            verdict = v == v1 ? 1 : 2;
        } else {
            const u64 epoch = (u64)(unsigned)I.misc[8] << 32;
            while ((v & 0xffffffff00000000ull) != epoch) { __builtin_amdgcn_s_sleep(8); v = gran_load(g); }
            verdict = (int)(v & 3ull);
        }
        if (lane == 0) { s_cnt[0] = verdict; s_cnt[1] = 0; s_cnt[2] = 0; }
    }
    for (int i = tid; i < E * 1024; i += 1024) { cnt[i] = 0; fill[i] = 0; }
    __syncthreads();
    if (s_cnt[0] != 1) return;                                                       // K5 proper ran (or runs): it builds the runs itself
    int hd[E], pdst[E];                                                              // pdst: where rank k's gradient goes (the plan)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * 1024 + tid;
        hd[e] = (k < n) ? rem_load(I.head, k) : -1;
        pdst[e] = (k < n) ? plan_dst(I, k) : 0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (hd[e] >= 0) atomicAdd(&cnt[hd[e]], 1);
        const u64 loose = __ballot(e * 1024 + tid < n && hd[e] < 0);
        if (lane == 0) nogroup[e * 16 + wave] = __builtin_popcountll(loose);
    }
    __syncthreads();
    if (wave == 0) {                                                                 // the plan's places for the ranks in no group: behind the runs, in rank order
        const int v = lane < E * 16 ? nogroup[lane] : 0;
        nogroup[lane] = (int)gnms_add_scan32((unsigned)v) - v;
    }
    // run starts: exclusive scan of the counts over the ranks (thread t owns ranks t * E .. t * E + E - 1)
    int c[E], sum = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) { c[e] = cnt[tid * E + e]; sum += c[e]; }
    const int inc = (int)gnms_add_scan32((unsigned)sum);
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 16; ++w) { const int v = wave_tot[w]; if (w < wave) base += v; total += v; }
    int run = base + inc - sum;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        startL[i] = run;
        if (i < n) { I.gstart[i] = run; I.glen[i] = c[e]; }
        // heads of multi-member groups -> hlist (any order), the big ones once more from the end (bwd_masked_*, solve_groups_kernel)
        const bool multi = i < n && c[e] > 1;
        const unsigned long long bm = __ballot(multi);
        if (bm) {
            int hb = 0;
            if (lane == __builtin_ctzll(bm)) hb = atomicAdd(&s_cnt[1], __builtin_popcountll(bm));
            hb = __builtin_amdgcn_readlane(hb, __builtin_ctzll(bm));
            if (multi) I.hlist[hb + __builtin_popcountll(bm & ((1ull << lane) - 1ull))] = i;
        }
        if (i < n && c[e] > kBigGroupList) I.hlist[N - 1 - atomicAdd(&s_cnt[2], 1)] = i;
        run += c[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) if (hd[e] >= 0) seg[startL[hd[e]] + atomicAdd(&fill[hd[e]], 1)] = e * 1024 + tid;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = e * 1024 + tid;
        const u64 loose = __ballot(k < n && hd[e] < 0);
        if (k >= N) continue;
        int pos = -1;
        if (hd[e] >= 0) {
            const int st = startL[hd[e]], len = cnt[hd[e]];
            pos = 0;
            for (int i = 0; i < len; ++i) pos += seg[st + i] < k ? 1 : 0;            // rank order inside the run, whatever order the atomics ran in
            I.gsorted[st + pos] = k;
            plan_entry(I, st + pos, k, pdst[e], pos, len, true);
        } else if (k < n) {
            plan_entry(I, total + nogroup[e * 16 + wave] + __builtin_popcountll(loose & ((1ull << lane) - 1ull)), k, pdst[e], 0, 0, false);
        } else {
            plan_pad(I, k);
        }
        I.gpos[k] = pos;
        if (k >= n) { I.head[k] = -1; I.glen[k] = 0; }                               // padding ranks: in no group
    }
    for (int i = total + tid; i < n; i += 1024) I.gsorted[i] = -1;                   // (behind the members, as K5's sort leaves it)
    if (tid == 0) { I.misc[1] = s_cnt[1]; I.misc[4] = s_cnt[2]; }
}

// ------------------------------------------------------------------------------------------------
// K3..K6 in ONE launch (masked groups): leaders -> attribution -> groups + rescoring -> finalize.  Chain workgroups per image: `spw` for
// the scan (the last one goes on with K4..K6), plus -- `fast` -- one for csr_build_body.
// Ppow2 >= 1024 (smaller images pad their keys).  dynamic LDS = max(leaders table (+ cnt), Ppow2 * 16).
// ------------------------------------------------------------------------------------------------
// is the fast tail possible for this launch? (decided on the host; the kernels get it as `fast`)
__host__ __device__ inline bool fast_tail_ok(int N, const gnms_params& P, int sym_arg, int chain_cap = 0) {
    return N <= 4096 && P.group_boxes && P.mask_group_boxes && !P.presorted && sym_arg != 0 && chain_cap == 0;
}

template <int E, int SRC>
__global__ __launch_bounds__(1024) void tail_kernel(const float* __restrict__ src, int N, long ld, const int* __restrict__ counts, gnms_params P,
                                                    char* ws, gnms_ws_layout L, int Ppow2, float* __restrict__ prob,
                                                    long long* __restrict__ valid, long long* __restrict__ invalid, int* __restrict__ nvalid,
                                                    int* __restrict__ ninvalid, int sym_arg, int B, int spw, int fast, int nchk) {
    int b;
    GNMS_TINIT();
    if constexpr (E <= 4) {
        if (fast) {
            // grid: [nchk symmetry checkers (sym_arg 3)] [B * spw scan workgroups] [B CSR workgroups]
            const int bx = (int)blockIdx.x - nchk;
            if (bx < 0) { wsym_check_in_launch(N, counts, ws, L, B, (int)blockIdx.x, nchk); return; }
            if (bx >= B * spw) {                                         // the image's CSR workgroup
                b = bx - B * spw;
                const int* misc = img_ptrs(ws, L, b).misc;
                const int symb = sym_arg == 2 ? (misc[3] == 0 ? 1 : 0) : (sym_arg == 3 ? (misc[2] == 0 ? 1 : 0) : sym_arg);
                if (symb) csr_build_body<E>(N, counts, ws, L, b);
                return;
            }
            int last = leaders_chain<SRC>(N, counts, ws, L, B, spw, bx, sym_arg, &b, src, ld, P.nms_threshold, P.temperature, P.pruning_method, Ppow2);
            if (!last) { GNMS_TFLUSH(ws, L, b); return; }
            if (last != 3 && sym_arg == 3) {                             // the scan ran on trust: the checkers' verdict before anything is final
                ImgPtrs I = img_ptrs(ws, L, b);
                int asym = 0;
                if (threadIdx.x < 64) {
                    while (__hip_atomic_load(I.misc + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nchk) __builtin_amdgcn_s_sleep(4);
                    asym = __hip_atomic_load(I.misc + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                }
                if (__syncthreads_or(asym)) {                            // not symmetric after all: the general scan, K4..K6 proper; nothing for the CSR workgroup
                    if (threadIdx.x == 0) gran_store(I.gran + (size_t)16 * 32 + kGranVerdict, ((u64)(unsigned)I.misc[8] << 32) | 2ull);
                    leaders_body(N, counts, ws, L, b);
                    last = 3;
                }
            }
            if (last != 3) { fast_final_body<E, SRC>(src, N, ld, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b, last); GNMS_TFLUSH(ws, L, b); return; }
            __syncthreads();                                             // general scan: K4..K6 as before
            attribute_image<SRC>(src, ld, N, counts, P.nms_threshold, ws, L, b, 0);
            __syncthreads();
            groups_body<E, SRC>(src, N, ld, counts, P, ws, L, Ppow2, b);
            __syncthreads();
            finalize_body<E>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
            return;
        }
    }
    if (!leaders_chain(N, counts, ws, L, B, spw, (int)blockIdx.x, sym_arg, &b)) return;   // (the image's other scan workgroups)
    const int sym = sym_arg == 2 ? (img_ptrs(ws, L, b).misc[3] == 0 ? 1 : 0) : sym_arg;   // (2: wsym_check_kernel's verdict for this image)
    __syncthreads();
    if (E <= 4 && sym && P.mask_group_boxes) {                       // the scan has attributed: K4's rest rides in K5, K6 starts from LDS
        if constexpr (E <= 4) {
            groups_body<E, SRC, true>(src, N, ld, counts, P, ws, L, Ppow2, b);
            lds_barrier();
            finalize_body<E, true>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
        }
        return;
    }
    attribute_image<SRC>(src, ld, N, counts, P.nms_threshold, ws, L, b, sym);
    __syncthreads();
    groups_body<E, SRC>(src, N, ld, counts, P, ws, L, Ppow2, b);
    __syncthreads();
    finalize_body<E>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
}

}  // namespace
}  // namespace gnms
