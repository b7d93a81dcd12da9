// gnms_device.h -- the device primitives the whole library borrows: coherent loads / stores, wave shuffles, the workgroup sorts
// (block_sort, block_radix_pass7), the per-image view of the workspace (ImgPtrs), single overlap entries (pair_iou, overlap_at), the small
// wave and flag helpers several stages of the NMS layer share, and the threshold guard band of the from-boxes decisions.
// __device__ / __host__ __device__ functions only: this header defines NO __global__ function, so a translation unit that includes it gets
// no kernel it does not launch.  The layer's kernels live in nms_sort_kernels.h (K1), nms_scan_kernels.h (K3) and nms_kernels.h (the rest).
#pragma once
#include "gnms_common.h"
#include "iou3d_pair.h"

namespace gnms {
namespace {   // internal linkage: the header is included by several translation units

typedef unsigned long long u64;

// Data that one workgroup of a launch hands to another workgroup of the SAME launch (the leader scan's granules and rem[], everything in
// one_launch_kernel): the L2s of the eight XCDs are not coherent with each other inside a kernel, so such data leaves through agent-scope
// (write-through) stores and is read with agent-scope loads.
template <typename T> __device__ __forceinline__ T coh_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ void coh_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float4 coh_load_f4(const float4* p) {
    const u64 a = coh_load(reinterpret_cast<const u64*>(p)), c = coh_load(reinterpret_cast<const u64*>(p) + 1);
    return make_float4(__uint_as_float((unsigned)a), __uint_as_float((unsigned)(a >> 32)), __uint_as_float((unsigned)c), __uint_as_float((unsigned)(c >> 32)));
}
__device__ __forceinline__ void coh_store_f4(float4* p, const float4 v) {
    coh_store(reinterpret_cast<u64*>(p), ((u64)__float_as_uint(v.y) << 32) | __float_as_uint(v.x));
    coh_store(reinterpret_cast<u64*>(p) + 1, ((u64)__float_as_uint(v.w) << 32) | __float_as_uint(v.z));
}

// lane ^ m / lane - off of a 64-bit (or 32-bit) value, as two 32-bit shuffles
__device__ __forceinline__ u64 shfl_xor_key(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), m, 64);
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ unsigned shfl_xor_key(unsigned v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int off) {
    const unsigned lo = __shfl_up((unsigned)(v & 0xffffffffu), off, 64);
    const unsigned hi = __shfl_up((unsigned)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------------
// block_sort: workgroup sort of P = blockDim.x * E 64-bit (or 32-bit) keys (P a power of two, blockDim.x a multiple of 64), ascending.
// Contract: thread t owns elements t*E .. t*E+E-1 in registers r[]; on return the sorted keys are in r[] AND in keys[0..P) (LDS, natural
// order), barrier included.
//   1. every wave sorts its own 64*E keys ascending with the register / shuffle part of a bitonic network (stages j < E in registers with
//      a compile-time partner, stages j < 64*E as wave shuffles, partner lane = lane ^ j/E);
//   2. the 64E-key runs are merged pairwise, log2(#waves) passes: each thread finds its E outputs by a merge-path
//      binary search on the two runs in LDS and merges them sequentially (ties take the left run).
// That replaces the 10 two-barrier LDS exchange stages + 24 shuffle stages above 64E of a pure bitonic network by
// 4 passes for 4096 keys (measured: 25 -> ~14 us for u64 keys on one CU).
// ------------------------------------------------------------------------------------------------
template <int E, typename K>
__device__ __forceinline__ void block_sort(K (&r)[E], K* keys, int P) {
    const int t = threadIdx.x;
    const int run = 64 * E < P ? 64 * E : P;                            // keys per wave-sorted run
    // ---- phase 1: wave-local bitonic sort (all runs ascending: the direction bit is dropped at k == run) ----
    for (int k = 2; k <= run; k <<= 1) {
        const int kd = (k == run) ? 0 : k;
        for (int j = k >> 1; j >= E; j >>= 1) {
            const int m = j / E;
            const bool keepmin = (((t * E) & kd) == 0) == (((t * E) & j) == 0);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const K o = shfl_xor_key(r[e], m);
                r[e] = ((o < r[e]) == keepmin) ? o : r[e];
            }
        }
#pragma unroll
        for (int jj = E / 2; jj >= 1; jj >>= 1) {
            if (jj < k) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & jj) == 0) {
                        const int i = t * E + e;
                        const bool up = (i & kd) == 0;
                        const K a = r[e], b = r[e | jj];
                        if ((a > b) == up) { r[e] = b; r[e | jj] = a; }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) keys[t * E + e] = r[e];
    __syncthreads();
    // ---- phase 2: pairwise merge passes ----
    for (int p = run; p < P; p <<= 1) {
        const int d0 = t * E;
        if (d0 >= P) { __syncthreads(); __syncthreads(); continue; }      // P < blockDim.x * E: the surplus threads only keep the barriers
        const int base = d0 & ~(2 * p - 1);
        const int d = d0 - base;                                        // diagonal inside the pair [A | B], |A| = |B| = p
        const K* A = keys + base;
        const K* Bk = keys + base + p;
        int lo = d > p ? d - p : 0, hi = d < p ? d : p;
        while (lo < hi) {                                               // merge path: first a with A[a] > B[d-1-a]
            const int mid = (lo + hi) >> 1;
            if (A[mid] <= Bk[d - 1 - mid]) lo = mid + 1; else hi = mid;
        }
        int a = lo, b = d - lo;
        K ka = a < p ? A[a] : K(0), kb = b < p ? Bk[b] : K(0);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool takeA = (b >= p) || (a < p && ka <= kb);
            r[e] = takeA ? ka : kb;
            if (takeA) { ++a; ka = a < p ? A[a] : K(0); } else { ++b; kb = b < p ? Bk[b] : K(0); }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) keys[t * E + e] = r[e];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Stable LSD radix pass over P = blockDim.x * E 32-bit keys in LDS, 7 bits per pass (128 digits), in place.
// Element order is the LDS order; wave w owns the 64*E consecutive slots [w*64E, (w+1)*64E), lane l reads slots e*64 + l
// (conflict-free), so a round e covers 64 consecutive elements and the stable rank inside the wave is
//   (same-digit elements of earlier rounds, kept in a per-wave histogram) + popcount(same-digit lanes below me),
// the same-digit lane mask coming from 7 ballots.  A (digit-major, wave-minor) exclusive scan of the 128 x #waves histogram
// gives every (wave, digit) its base.  5 barriers per pass; 2 passes sort 14-bit keys (the groups' leader ranks), where the
// merge-path block_sort needs ~15 us for 4096 keys and this needs ~4.
// hist: 128 * (blockDim.x / 64) + 16 unsigned words of LDS.
// ------------------------------------------------------------------------------------------------
template <int E>
__device__ __forceinline__ void block_radix_pass7(unsigned* keys, int shift, unsigned* hist) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
    unsigned* wtot = hist + 128 * nw;
    for (int i = t; i < 128 * nw; i += blockDim.x) hist[i] = 0u;
    unsigned k[E], rnk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) k[e] = keys[wave * 64 * E + e * 64 + lane];
    __syncthreads();
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned d = (k[e] >> shift) & 127u;
        u64 same = ~0ull;
#pragma unroll
        for (int bit = 0; bit < 7; ++bit) {
            const bool on = (d >> bit) & 1u;
            const u64 bl = __ballot(on);
            same &= on ? bl : ~bl;
        }
        const unsigned prior = hist[wave * 128 + d];
        rnk[e] = prior + (unsigned)__builtin_popcountll(same & below);
        if ((same & below) == 0ull) hist[wave * 128 + d] = prior + (unsigned)__builtin_popcountll(same);   // the digit's lowest lane
        __builtin_amdgcn_wave_barrier();                                // the next round reads what this one wrote (same wave: in order)
    }
    __syncthreads();
    // exclusive scan in (digit, wave) order: entry j = d * nw + w lives at hist[w * 128 + d]; thread t owns j = 2t, 2t + 1
    const int j0 = 2 * t, j1 = 2 * t + 1;
    const int lw = 31 - __builtin_clz(nw);                               // #waves is a power of two
    const int a0 = (j0 & (nw - 1)) * 128 + (j0 >> lw), a1 = (j1 & (nw - 1)) * 128 + (j1 >> lw);
    const unsigned c0 = hist[a0], c1 = hist[a1];
    const unsigned inc = gnms_add_scan32(c0 + c1);                       // DPP prefix sum: no ds_bpermute round trips
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    // sum of the totals of the waves before mine (<= 16 of them): lane w < wave holds total w, lane 63 of the scan has the sum
    const unsigned carry = (unsigned)__builtin_amdgcn_readlane((int)gnms_add_scan32((lane < wave) ? wtot[lane] : 0u), 63);
    const unsigned ex = carry + inc - (c0 + c1);
    hist[a0] = ex;
    hist[a1] = ex + c0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) keys[hist[wave * 128 + ((k[e] >> shift) & 127u)] + rnk[e]] = k[e];
    __syncthreads();
}

template <typename K>
__device__ __forceinline__ int lower_bound_lds(const K* keys, int n, K v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct ImgPtrs {
    int* order; float* sscore; int* rankof; int* rem; int* head; int* gpos; int* gsorted; int* gstart; int* glen; int* hlist;
    float* plead; float* pre; float* r2; int* sidx; float* xsol; float* gx; int* leadc; int* leadr; u64* leadw; int* leadpfx;
    int* misc; u64* gran; int* xidx; float4* xbox; float4* rbox; float* rec; float* xrec; u64* plan; u64* W;
};

__device__ __host__ __forceinline__ ImgPtrs img_ptrs(char* ws, const gnms_ws_layout& L, int b) {
    char* p = ws + (size_t)b * L.per_image;
    ImgPtrs I;
    I.order = (int*)(p + L.off_order); I.sscore = (float*)(p + L.off_sscore); I.rankof = (int*)(p + L.off_rankof); I.rem = (int*)(p + L.off_rem);
    I.head = (int*)(p + L.off_head); I.gpos = (int*)(p + L.off_gpos); I.gsorted = (int*)(p + L.off_gsorted);
    I.gstart = (int*)(p + L.off_gstart); I.glen = (int*)(p + L.off_glen); I.hlist = (int*)(p + L.off_hlist); I.plead = (float*)(p + L.off_plead);
    I.pre = (float*)(p + L.off_pre); I.r2 = (float*)(p + L.off_r2); I.sidx = (int*)(p + L.off_sidx);
    I.xsol = (float*)(p + L.off_xsol); I.gx = (float*)(p + L.off_gx); I.leadc = (int*)(p + L.off_leadc); I.leadr = (int*)(p + L.off_leadr);
    I.leadw = (u64*)(p + L.off_leadw); I.leadpfx = (int*)(p + L.off_leadpfx); I.misc = (int*)(p + L.off_misc);
    I.gran = (u64*)(p + L.off_gran); I.xidx = (int*)(p + L.off_xidx); I.xbox = (float4*)(p + L.off_xbox); I.rbox = (float4*)(p + L.off_rbox); I.rec = (float*)(p + L.off_rec); I.xrec = (float*)(p + L.off_xrec);
    I.plan = (u64*)(p + L.off_plan);
    I.W = (u64*)(p + L.off_W);
    return I;
}

// IoU of box a (row) against box b (column): the arithmetic of iou2d_kernel / lib/core.py:210-218,499-508, operation
// for operation, so that the from-boxes path takes exactly the decisions the matrix path takes.
__device__ __forceinline__ float pair_iou(const float4 a, const float4 b) {
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f);
    const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
    const float inter = w * h;
    return inter / ((area_a + area_b) - inter);
}

// element [ca][cb] (input indices) of the overlaps' source SRC (kFromMatrix / kFromBoxes / kFromRecords: gnms_common.h)
// thr: the layer's nms_threshold (records only: entries inside the guard band around it take the reference's exact order, iou3d_pair.h)
template <int SRC>
__device__ __forceinline__ float overlap_at(const float* __restrict__ src, long ld, int ca, int cb, float thr) {
    if (SRC == kFromBoxes) {
        const float4* bx = reinterpret_cast<const float4*>(src);
        return pair_iou(bx[ca], bx[cb]);
    }
    if (SRC == kFromRecords) return gnms_iou3d::nms_overlap3d_pair(src + (size_t)ca * gnms_iou3d::kRec, src + (size_t)cb * gnms_iou3d::kRec, thr);
    return src[(size_t)ca * ld + cb];
}

// the image's slice of what the caller passed as `src` (records live in the workspace, not in a caller array)
template <int SRC>
__device__ __forceinline__ const float* overlap_src(const float* __restrict__ src, const ImgPtrs& I, int b, int N, long ld) {
    if (SRC == kFromRecords) return I.rec;
    return src + (SRC == kFromBoxes ? (size_t)b * N * 4 : (size_t)b * N * ld);
}

// ------------------------------------------------------------------------------------------------
// Small wave and flag helpers that several stages share
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_min_f(float v) { return gnms_wave_min_f(v); }   // DPP network: no ds_bpermute round trips
__device__ __forceinline__ float wave_max_f(float v) { return gnms_wave_max_f(v); }

__device__ __forceinline__ float4 load_nt_f4(const float* p) {
    float4 v;
    v.x = __builtin_nontemporal_load(p);
    v.y = __builtin_nontemporal_load(p + 1);
    v.z = __builtin_nontemporal_load(p + 2);
    v.w = __builtin_nontemporal_load(p + 3);
    return v;
}

// workgroup barrier that waits for this wave's LDS operations only (not for its global loads / stores, as __syncthreads does): for
// hand-offs that live in LDS.  Beside the matrix writers the drain of a wave's stores takes microseconds.
// (LDS-only fences around the barrier builtin, not inline asm with a "memory" clobber: behind the clobber the compiler re-derived
// everything it had loaded from memory -- kernel arguments, counts[b] -- after EVERY barrier, ~1000 cycles per step of a loop of them)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)(v & 0xffffffffu), lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// Flags of the one launch (nms_one_launch.h): a granule that is valid only with the launch's tag AND its own slot number, so that no stale
// or foreign word can pass for it.  The slot numbers:
__device__ __forceinline__ u64 strong_gran(unsigned tag, unsigned slot) { return ((u64)tag << 32) | (u64)(unsigned)(~tag ^ (0x9E3779B9u * (slot + 1u))); }
constexpr unsigned kSlotSort = 0u;       // + 32 * role + workgroup of the sort          -> gran[1 + role][workgroup]
constexpr unsigned kSlotBits = 64u;      // + workgroup of the bit table (<= 416)        -> gran[3 .. 15][workgroup]
constexpr unsigned kSlotVerdict = 512u;  // + the verdict (1 fast tail, 2 K5 proper ran) -> gran[16][kGranVerdict]

// The leader scan's hand-off granules (nms_scan_kernels.h, HAND-OFF): single write-through stores, polled with agent-scope loads
__device__ __forceinline__ u64 gran_load(const u64* p) {
    return (u64)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gran_store(u64* p, u64 v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// rem[] as the leader scan leaves it: agent-scope accesses (plain ones would do between kernels, these do everywhere)
__device__ __forceinline__ int rem_load(const int* rem, int k) { return __hip_atomic_load(rem + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rem_store(int* rem, int k, int v) { __hip_atomic_store(rem + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------------
// The threshold guard band of the from-boxes decisions: !(fl(inter/uni) <= thr) WITHOUT the division.
// With d = fma(-thr, uni, inter) (one rounding, sign exact):
//   inter/uni - thr = d/uni,  so  |d| > band*uni  puts the exact quotient more than `band` (8 ulp of the threshold)
// away from thr, hence its fp32 rounding on the same side, and the pair is decided by the sign of d.  That needs
// uni > 0 and finite, which holds whenever both boxes have a positive finite area (inter <= min(area) in fp32 as in
// exact arithmetic because subtraction/multiplication round monotonically, so uni >= max(area) > 0).  Boxes that fail that,
// and the pairs inside the band, take the exact IEEE division.  Every kernel that decides this way takes the band from here, so that
// all of them take the same decisions: bitmask_boxes_body (packed and scalar rows), one_launch_bits_from_boxes(_x), classic_mask_kernel,
// classic_ext_kernel.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float iou_guard_band(float thr) { return fmaxf(fabsf(thr), 1.0f) * 9.6e-7f; }   // 8 ulp at the threshold's magnitude (>= 1 for tiny thresholds)

// The scalar general row: one row box (ax1, ay1, ax2, ay2) of area aa, broadcast from SGPRs, against the lane's column box cb of area
// carea -> inter, uni, d = fma(-thr, uni, inter).  The arithmetic of pair_iou up to the division (row box is `a`, column box is `b`).
// The band test, the wave vote and the choice between division and sign stay with the caller.
// (v_min / v_max issued directly, the row coordinate straight from its SGPR: fminf / fmaxf on loaded values cost a canonicalising
// v_max x, x each -- 12 of the ~85 VALU instructions of a row; same values, iou3d_pair.h)
__device__ __forceinline__ void iou_row_terms(float ax1, float ay1, float ax2, float ay2, float aa, const float4 cb, float carea, float thr,
                                              float& inter, float& uni, float& d) {
    const float w = fmaxf(gnms_iou3d::vmin_s(ax2, cb.z) - gnms_iou3d::vmax_s(ax1, cb.x), 0.0f);
    const float h = fmaxf(gnms_iou3d::vmin_s(ay2, cb.w) - gnms_iou3d::vmax_s(ay1, cb.y), 0.0f);
    inter = w * h;
    uni = (aa + carea) - inter;
    d = __builtin_fmaf(-thr, uni, inter);
}

}  // namespace
}  // namespace gnms
