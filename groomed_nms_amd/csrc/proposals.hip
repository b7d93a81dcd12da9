// proposals.hip -- what sits directly in front of the NMS layer: box decode and the score top-K that picks
// the boxes the layer sees, on the device, so that scores/boxes never bounce through host NumPy.
//
// Reference:
//   lib/rpn_util.py:872-934      bbox_transform_inv      anchors + deltas (de-normalised by stds/means) -> x1 y1 x2 y2
//   lib/loss/rpn_3d.py:731-737   torch.sort(scores[fg], descending) -> the first min(500, #fg) foreground boxes go to the NMS
//   lib/rpn_util.py:1258-1266    the same selection at inference (argsort of -score, first nms_topN)
// The reference's selection then goes through .cpu()/.numpy() (rpn_3d.py:740-744); here it stays in HBM: gnms_select_topk
// emits the indices AND the gathered scores/boxes in the padded [B][K] layout gnms_forward_with_iou2d consumes.
#include <algorithm>
#include <map>
#include <mutex>
#include "gnms_device.h"
#include "bbox_decode.h"

namespace {

using namespace gnms;

// lib/rpn_util.py:886-927, same operation order
__global__ __launch_bounds__(256) void bbox_transform_inv_kernel(const float4* __restrict__ anchors, const float4* __restrict__ deltas, long A,
                                                                 long total, float4 means, float4 stds, int use_means, int use_stds,
                                                                 float4* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    out[i] = gnms_bbox_decode(anchors[i % A], deltas[i], means, stds, use_means, use_stds);   // (bbox_decode.h: shared with detect3d.hip)
}

// One workgroup per image: stable descending sort of the candidates' scores, the first min(K, #candidates) leave.
template <int E>
__global__ __launch_bounds__(1024) void select_topk_kernel(const float* __restrict__ scores, int A, const int* __restrict__ cand, int F,
                                                           const int* __restrict__ cand_counts, int K, int P,
                                                           const float4* __restrict__ boxes, long long* __restrict__ sel_idx,
                                                           int* __restrict__ sel_count, float* __restrict__ sel_scores,
                                                           float4* __restrict__ sel_boxes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    const int b = blockIdx.x;
    const int f = gnms_count(cand_counts, b, F);
    const float* s = scores + (size_t)b * A;
    const int* cd = cand ? cand + (size_t)b * F : nullptr;
    u64 r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = threadIdx.x * E + e;
        r[e] = ~0ull;
        if (i < f) {
            int a = cd ? cd[i] : i;
            a = a < 0 ? 0 : (a >= A ? A - 1 : a);                       // a bad index must not turn into an out-of-bounds read
            r[e] = ((u64)gnms_desc_key(s[a]) << 32) | (unsigned)i;      // ties: the earlier candidate first
        }
    }
    block_sort<E, u64>(r, keys, P);
    const int m = f < K ? f : K;
    if (threadIdx.x == 0 && sel_count) sel_count[b] = m;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        long long idx = -1;
        float sc = 0.0f;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < m) {
            const int i = (int)(keys[k] & 0xffffffffu);
            int a = cd ? cd[i] : i;
            a = a < 0 ? 0 : (a >= A ? A - 1 : a);
            idx = a;
            sc = s[a];
            if (boxes) bx = boxes[(size_t)b * A + a];
        }
        if (sel_idx) sel_idx[(size_t)b * K + k] = idx;                  // padded with -1 / 0 behind the count
        if (sel_scores) sel_scores[(size_t)b * K + k] = sc;
        if (sel_boxes) sel_boxes[(size_t)b * K + k] = bx;
    }
}

// MORE candidates than one workgroup sorts in LDS (> GNMS_MAX_BOXES; the reference's inference path selects among ALL anchors,
// lib/rpn_util.py:1258-1266: ~127k per image): a pre-selection that leaves exactly the K candidates the stable descending sort would put
// first, in their original order, for select_topk_kernel to sort.  One workgroup per image:
//   1. radix select on the 32-bit descending key, 8 bits per pass from the top (LDS histogram of the keys that match the prefix so far):
//      T = the K-th smallest key, need_eq = how many keys equal to T still belong to the first K;
//   2. compaction in candidate order: keys < T, and the first need_eq keys == T (ties: the earlier candidate, as a stable sort has it) --
//      every thread owns a contiguous chunk, two block scans (smaller / equal) give its output offsets.
__global__ __launch_bounds__(1024) void topk_preselect_kernel(const float* __restrict__ scores, int A, const int* __restrict__ cand, int F,
                                                              const int* __restrict__ cand_counts, int K, int* __restrict__ out_cand,
                                                              int* __restrict__ out_count) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_need;
    __shared__ int wsum_lt[16], wsum_eq[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = gnms_count(cand_counts, b, F);
    const float* s = scores + (size_t)b * A;
    const int* cd = cand ? cand + (size_t)b * F : nullptr;
    auto key_of = [&](int i) {
        int a = cd ? cd[i] : i;
        a = a < 0 ? 0 : (a >= A ? A - 1 : a);
        return gnms_desc_key(s[a]);
    };
    int* oc = out_cand + (size_t)b * K;
    if (f <= K) {                                                    // everything is selected
        for (int i = tid; i < f; i += 1024) oc[i] = cd ? cd[i] : i;
        if (tid == 0) out_count[b] = f;
        return;
    }
    if (tid == 0) { s_prefix = 0u; s_need = (unsigned)K; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += 1024) hist[i] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix;
        const unsigned himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        // (a thread adds a run of equal digits at once: scores of one sign share their top byte, and 127k single increments of ONE
        // LDS word serialise)
        unsigned run_d = 0u, run_n = 0u;
        for (int i0 = tid; i0 < f; i0 += 8 * 1024) {                  // eight loads in flight per thread: the pass is latency-bound
            unsigned k8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) k8[u] = (i0 + u * 1024 < f) ? key_of(i0 + u * 1024) : 0u;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u * 1024 < f && (k8[u] & himask) == prefix) {
                    const unsigned d = (k8[u] >> shift) & 255u;
                    if (d == run_d) ++run_n;
                    else { if (run_n) atomicAdd(&hist[run_d], run_n); run_d = d; run_n = 1u; }
                }
            }
        }
        if (run_n) atomicAdd(&hist[run_d], run_n);
        __syncthreads();
        if (wave == 0) {                                             // the digit that holds the need-th smallest key with this prefix
            const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const unsigned mine = h0 + h1 + h2 + h3;
            const unsigned inc = gnms_add_scan32(mine);               // bins 0 .. 4 lane + 3
            const unsigned need = s_need;
            const u64 reach = __ballot(inc >= need);                  // (the last lane always reaches: need <= #keys with this prefix)
            const int l = __builtin_ctzll(reach);
            if (lane == l) {
                unsigned rest = need - (inc - mine), d = 4u * lane;
                if (rest > h0) { rest -= h0; ++d; if (rest > h1) { rest -= h1; ++d; if (rest > h2) { rest -= h2; ++d; } } }
                s_prefix = prefix | (d << shift);
                s_need = rest;
            }
        }
        __syncthreads();
    }
    const unsigned T = s_prefix, need_eq = s_need;                   // keys < T all belong; of the keys == T the first need_eq
    // compaction in candidate order, coalesced: wave w owns the contiguous range [w * per, (w + 1) * per), 64 candidates per trip
    const int per = ((f + 15) / 16 + 63) & ~63;
    const int w0 = wave * per, w1 = min(f, w0 + per);
    int nlt = 0, neq = 0;
    for (int i = w0 + lane; i - lane < w1; i += 64) {
        const unsigned k = i < w1 ? key_of(i) : 0xffffffffu;
        nlt += __builtin_popcountll(__ballot(i < w1 && k < T));
        neq += __builtin_popcountll(__ballot(i < w1 && k == T));
    }
    if (lane == 0) { wsum_lt[wave] = nlt; wsum_eq[wave] = neq; }
    __syncthreads();
    int lt = 0, eq = 0;
    for (int w = 0; w < wave; ++w) { lt += wsum_lt[w]; eq += wsum_eq[w]; }
    // output position of a selected candidate = (# smaller before it) + (# selected equal before it), both in candidate order
    const u64 below = (1ull << lane) - 1ull;
    for (int i = w0 + lane; i - lane < w1; i += 64) {
        const unsigned k = i < w1 ? key_of(i) : 0xffffffffu;
        const bool is_lt = i < w1 && k < T, is_eq = i < w1 && k == T;
        const u64 b_lt = __ballot(is_lt), b_eq = __ballot(is_eq);
        const int lt_me = lt + __builtin_popcountll(b_lt & below), eq_me = eq + __builtin_popcountll(b_eq & below);
        if (is_lt) oc[lt_me + min(eq_me, (int)need_eq)] = cd ? cd[i] : i;
        else if (is_eq && eq_me < (int)need_eq) oc[lt_me + eq_me] = cd ? cd[i] : i;
        lt += __builtin_popcountll(b_lt);
        eq += __builtin_popcountll(b_eq);
    }
    if (tid == 0) out_count[b] = K;
}

// ------------------------------------------------------------------------------------------------
// Top-K over SEVERAL workgroups per image (round 5; VERDICT r4 #4b).  One workgroup per image read the ~127 k anchors of an inference image
// six times through one CU (four histogram passes + two compaction passes) and then sorted the K survivors alone: 96 us for the top 4096
// of 16 384, more for all anchors.  Here G workgroups per image run ONE cooperative launch (B * G <= CUs: every workgroup is resident, so
// they may wait for each other):
//   load     a thread keeps its (up to) kCoopKPT keys in REGISTERS for the whole launch -- the scores are read once;
//   select   radix select of the K-th smallest descending key, three digits of 11 / 11 / 10 bits: LDS histogram of the keys that match the
//            prefix, non-empty bins added to the image's global histogram, a grid barrier, every workgroup finds the digit for itself;
//   ties     keys equal to the threshold are taken in candidate order (what a stable sort does): per-workgroup counts, a barrier, prefix;
//   sort     the K selected (key, candidate position) pairs: workgroup r sorts run r (1024 pairs) in LDS, a barrier, then ranks its run
//            against all runs (binary searches, the rank merge of sort_merge_body) and emits indices, scores and boxes at the final
//            positions, padding included.
// A grid barrier = one device-scope atomic increment per workgroup and a poll (~2.5 us); six of them.  Data that crosses workgroups
// (histograms, counts, the selected pairs, the sorted runs) moves through device-scope atomics / agent-scope loads and stores.
// ------------------------------------------------------------------------------------------------
constexpr int kCoopKPT = 8;                       // keys per thread
constexpr int kCoopChunk = 1024 * kCoopKPT;       // candidates per workgroup
constexpr int kCoopBins = 2048;
struct CoopScratch {                              // the part of an image's scratch that every launch must FIND ZEROED
    unsigned hist[3][kCoopBins];
    unsigned bar[8];
    unsigned sel_count;
    unsigned exits;                               // workgroups of the image that are done: the last one zeroes this struct again
    unsigned pad[6];
};
// One scratch per device, kept between the calls (launches of this kernel are chained across streams, see gnms_select_topk: never two at
// once): kCoopMaxImages headers first -- at the same place whatever G and K a call has, each left zeroed by the image's last workgroup --
// then per image  unsigned cnt[G][2]; u64 sel[Kpad]; u64 runs[Kpad]  (written before they are read: any content will do).
// Round 5, first version: a stream-ordered temporary + a memset per call, 5 us on the device and three more API calls on the host.
constexpr int kCoopMaxImages = 512;
__host__ __device__ inline size_t coop_rest_bytes(int G, int Kpad) { return ((size_t)G * 2 * sizeof(unsigned) + 15) / 16 * 16 + (size_t)Kpad * 16; }
__host__ __device__ inline size_t coop_scratch_bytes(int B, int G, int Kpad) {
    return (size_t)kCoopMaxImages * sizeof(CoopScratch) + (size_t)B * coop_rest_bytes(G, Kpad);
}

__device__ __forceinline__ void coop_grid_barrier(unsigned* counter, const unsigned G) {
    __builtin_amdgcn_s_waitcnt(0x0f70);                               // vmcnt(0): this wave's stores / atomics are out
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // The host only launches this kernel when every workgroup of the grid is resident at once (gnms_select_topk: occupancy x CUs >= B * G,
        // launches of this kind chained across streams).  What the host cannot see -- another PROCESS holding CUs, a CU-masked stream -- would
        // make this wait for ever and hang the GPU; a wait of two seconds (s_memtime: 100 MHz) aborts the launch instead, which the next
        // synchronisation reports as an error.
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        unsigned polls = 0;
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < G) {
            __builtin_amdgcn_s_sleep(2);
            if ((++polls & 0xfffu) == 0u && __builtin_amdgcn_s_memtime() - t0 > 200000000ull) __builtin_trap();
        }
    }
    __syncthreads();
}

// the digit of the (need)-th smallest key among the bins of one global histogram; every thread returns the same (digit, rest)
__device__ __forceinline__ void coop_find_digit(const unsigned* hist, const int nbins, const unsigned need, unsigned* digit, unsigned* rest,
                                                unsigned* binc, unsigned* wtot /* [16] LDS */, unsigned* out2 /* [3] LDS */) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // thread t owns bins 2 t, 2 t + 1 (nbins <= 2048)
    const unsigned h0 = (2 * t < nbins) ? __hip_atomic_load(hist + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned h1 = (2 * t + 1 < nbins) ? __hip_atomic_load(hist + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned mine = h0 + h1;
    const unsigned inc = gnms_add_scan32(mine);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned base = 0u;
    for (int w = 0; w < wave; ++w) base += wtot[w];
    const unsigned before = base + inc - mine;                        // keys in bins < 2 t
    if (before < need && need <= before + mine) {                     // exactly one thread (need >= 1, need <= total)
        unsigned d = 2u * t, r = need - before, c = h0;
        if (r > h0) { r -= h0; ++d; c = h1; }
        out2[0] = d; out2[1] = r; out2[2] = c;
    }
    __syncthreads();
    *digit = out2[0];
    *rest = out2[1];
    *binc = out2[2];                                                  // keys in the chosen bin
    __syncthreads();
}

__global__ __launch_bounds__(1024) void topk_coop_kernel(const float* __restrict__ scores, int A, const int* __restrict__ cand, int F,
                                                         const int* __restrict__ cand_counts, int K, int Kpad, int G, char* scratch_all,
                                                         const float4* __restrict__ boxes, long long* __restrict__ sel_idx,
                                                         int* __restrict__ sel_count, float* __restrict__ sel_scores, float4* __restrict__ sel_boxes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* lh = reinterpret_cast<unsigned*>(smem);                  // [2048] LDS histogram; later the sort's keys
    __shared__ unsigned wtot[16], out2[4];
    const int g = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = gnms_count(cand_counts, b, F);
    const float* s = scores + (size_t)b * A;
    const int* cd = cand ? cand + (size_t)b * F : nullptr;
    CoopScratch* S = reinterpret_cast<CoopScratch*>(scratch_all) + b;
    char* sp = scratch_all + (size_t)kCoopMaxImages * sizeof(CoopScratch) + (size_t)b * coop_rest_bytes(G, Kpad);
    unsigned* cnt = reinterpret_cast<unsigned*>(sp);                                           // [G][2]: keys below / equal to the threshold
    u64* sel = reinterpret_cast<u64*>(sp + ((size_t)G * 2 * sizeof(unsigned) + 15) / 16 * 16);   // [Kpad]
    u64* runs = sel + Kpad;                                                                   // [Kpad] sorted runs of 1024
    const int m = f < K ? f : K;                                       // boxes selected
    auto index_of = [&](int i) { int a = cd ? cd[i] : i; return a < 0 ? 0 : (a >= A ? A - 1 : a); };   // (a bad index must not read out of bounds)
    // ---- load: candidate i = g * chunk + e * 1024 + t ----
    unsigned key[kCoopKPT];
    const int i0 = g * kCoopChunk + t;
#pragma unroll
    for (int e = 0; e < kCoopKPT; ++e) {
        const int i = i0 + e * 1024;
        key[e] = (i < f) ? gnms_desc_key(s[index_of(i)]) : 0xffffffffu;          // (a real key can be 0xffffffff too: validity is i < f, not the key)
    }
    unsigned eq_total = 0u;
    unsigned T = 0xffffffffu, need_eq = 0u;                            // keys < T are all selected; of the keys == T the first need_eq (candidate order)
    bool all = f <= K;                                                 // everything is selected
    if (!all) {
        unsigned prefix = 0u, need = (unsigned)K;
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0), nb = pass == 2 ? 1024 : kCoopBins;
            const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (pass == 1 ? 21 : 10));
            for (int i = t; i < nb; i += 1024) lh[i] = 0u;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kCoopKPT; ++e)
                if (i0 + e * 1024 < f && (key[e] & himask) == prefix) atomicAdd(&lh[(key[e] >> shift) & (unsigned)(nb - 1)], 1u);
            __syncthreads();
            for (int i = t; i < nb; i += 1024) { const unsigned v = lh[i]; if (v) __hip_atomic_fetch_add(&S->hist[pass][i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            coop_grid_barrier(&S->bar[pass], (unsigned)G);
            unsigned d, rest;
            coop_find_digit(S->hist[pass], nb, need, &d, &rest, &eq_total, wtot, out2);
            prefix |= d << shift;
            need = rest;
        }
        T = prefix;
        need_eq = need;                                                // (eq_total: the last pass's bin is ONE key value: the keys equal to T)
    }
    // ---- which keys equal to T belong: per-workgroup counts, prefix over the workgroups before mine ----
    // (only when SOME of the keys equal to T belong -- the same decision in every workgroup, from the same histogram: otherwise all of them
    // are taken, nobody needs anybody's counts, and a grid barrier is saved: the common case, a threshold that one key holds)
    const bool take_all_eq = !all && need_eq >= eq_total;
    unsigned eq_before = 0u;                                           // keys == T in the workgroups before mine (candidate order)
    unsigned eq_mine = 0u;                                             // ... and in this workgroup
    if (!all && !take_all_eq) {
        unsigned neq = 0u;
#pragma unroll
        for (int e = 0; e < kCoopKPT; ++e) neq += __builtin_popcountll(__ballot(i0 + e * 1024 < f && key[e] == T));
        if (lane == 0) wtot[wave] = neq;
        __syncthreads();
        unsigned weq = 0u;
        for (int w = 0; w < 16; ++w) weq += wtot[w];
        eq_mine = weq;
        if (t == 0) __hip_atomic_store(cnt + 2 * g + 1, weq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        coop_grid_barrier(&S->bar[3], (unsigned)G);
        for (int w = 0; w < g; ++w) eq_before += __hip_atomic_load(cnt + 2 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the selected pairs (key << 32 | candidate position) into sel[], any order: the sort below orders them ----
    // Two passes: which of the thread's keys are taken (LDS only), then ONE device-scope fetch-add per workgroup for its range of sel[]
    // and the stores.  (Round 5, first version: a returning fetch-add per wave and round of keys -- eight dependent memory round trips.)
    {
        unsigned takemask = 0u, wave_take = 0u;
        unsigned eq_run = eq_before;                                   // keys == T in front of (e, wave 0 lane 0), candidate order
#pragma unroll
        for (int e = 0; e < kCoopKPT; ++e) {
            const int i = i0 + e * 1024;
            const bool v = i < f;
            bool take = v && (all || key[e] < T || (take_all_eq && key[e] == T));
            if (eq_mine != 0u) {                                       // (workgroup-uniform: keys equal to the threshold are rare)
                const bool is_eq = v && !all && key[e] == T;
                const u64 beq = __ballot(is_eq);
                // candidate order inside the workgroup is (e, t): the equal keys of the waves before mine in this round, then the lanes before me
                if (lane == 0) wtot[wave] = (unsigned)__builtin_popcountll(beq);
                __syncthreads();
                unsigned wbefore = 0u, wall = 0u;
                for (int w = 0; w < 16; ++w) { const unsigned c = wtot[w]; if (w < wave) wbefore += c; wall += c; }
                __syncthreads();
                const unsigned my_eq = eq_run + wbefore + (unsigned)__builtin_popcountll(beq & ((1ull << lane) - 1ull));
                take = take || (is_eq && my_eq < need_eq);
                eq_run += wall;
            }
            takemask |= take ? (1u << e) : 0u;
            wave_take += (unsigned)__builtin_popcountll(__ballot(take));
        }
        if (lane == 0) wtot[wave] = wave_take;
        __syncthreads();
        unsigned run = 0u, wg_take = 0u;
        for (int w = 0; w < 16; ++w) { const unsigned c = wtot[w]; if (w < wave) run += c; wg_take += c; }
        if (t == 0) out2[0] = wg_take ? __hip_atomic_fetch_add(&S->sel_count, wg_take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        __syncthreads();
        run += out2[0];
#pragma unroll
        for (int e = 0; e < kCoopKPT; ++e) {
            const bool take = (takemask >> e) & 1u;
            const u64 bt = __ballot(take);
            const unsigned pos = run + (unsigned)__builtin_popcountll(bt & ((1ull << lane) - 1ull));
            if (take && pos < (unsigned)Kpad)
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(sel + pos), ((unsigned long long)key[e] << 32) | (unsigned)(i0 + e * 1024),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            run += (unsigned)__builtin_popcountll(bt);
        }
    }
    coop_grid_barrier(&S->bar[4], (unsigned)G);
    // ---- sort: run r by workgroup r, then the rank merge ----
    const int R = (m + 1023) >> 10;                                    // runs of 1024 (m <= Kpad)
    u64* keys = reinterpret_cast<u64*>(smem);                          // [R][1024] (R <= 16)
    if (g < R) {
        u64 r1[1];
        const int i = g * 1024 + t;
        r1[0] = (i < m) ? (u64)__hip_atomic_load(reinterpret_cast<unsigned long long*>(sel + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
        block_sort<1, u64>(r1, keys, 1024);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(runs + i), (unsigned long long)r1[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    coop_grid_barrier(&S->bar[5], (unsigned)G);
    if (g == 0 && t == 0 && sel_count) sel_count[b] = m;
    if (g < R) {
        for (int q = 0; q < R; ++q)
            keys[q * 1024 + t] = (u64)__hip_atomic_load(reinterpret_cast<unsigned long long*>(runs + q * 1024 + t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const u64 mine = keys[g * 1024 + t];
        if (mine != ~0ull) {
            int rank = 0;
            for (int q = 0; q < R; ++q) rank += (q == g) ? t : lower_bound_lds<u64>(keys + q * 1024, 1024, mine);
            const int i = (int)(mine & 0xffffffffu), a = index_of(i);
            if (sel_idx) sel_idx[(size_t)b * K + rank] = a;
            if (sel_scores) sel_scores[(size_t)b * K + rank] = s[a];
            if (sel_boxes) sel_boxes[(size_t)b * K + rank] = boxes[(size_t)b * A + a];
        }
    }
    // padding behind the count: -1 / 0 (the padded layout gnms_forward_with_iou2d takes with counts)
    for (int k = m + g * 1024 + t; k < K; k += G * 1024) {
        if (sel_idx) sel_idx[(size_t)b * K + k] = -1;
        if (sel_scores) sel_scores[(size_t)b * K + k] = 0.0f;
        if (sel_boxes) sel_boxes[(size_t)b * K + k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the image's last workgroup to get here leaves the header zeroed for the next call (every other one is behind its last barrier and its
    // last read of the histograms: nobody looks at the header any more)
    __shared__ unsigned last_one;
    __syncthreads();
    if (t == 0) last_one = __hip_atomic_fetch_add(&S->exits, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(G - 1);
    __syncthreads();
    if (last_one) {
        unsigned* z = reinterpret_cast<unsigned*>(S);
        for (int i = t; i < (int)(sizeof(CoopScratch) / sizeof(unsigned)); i += 1024) __hip_atomic_store(z + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int next_pow2(int n) {
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" int gnms_bbox_transform_inv(const float* anchors, const float* deltas, int B, int A, const float* means, const float* stds,
                                       float* out, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && A >= 0, "gnms_bbox_transform_inv: negative size");
    if (B == 0 || A == 0) return GNMS_OK;
    GNMS_CHECK_ARG(anchors && deltas && out, "gnms_bbox_transform_inv: null pointer");
    GNMS_CHECK_ARG(((uintptr_t)anchors % 16 == 0) && ((uintptr_t)deltas % 16 == 0) && ((uintptr_t)out % 16 == 0),
                   "gnms_bbox_transform_inv: pointers must be 16-byte aligned");
    const float4 m = means ? make_float4(means[0], means[1], means[2], means[3]) : make_float4(0.f, 0.f, 0.f, 0.f);   // host pointers
    const float4 s = stds ? make_float4(stds[0], stds[1], stds[2], stds[3]) : make_float4(1.f, 1.f, 1.f, 1.f);
    const long total = (long)B * A;
    bbox_transform_inv_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(anchors), reinterpret_cast<const float4*>(deltas), (long)A, total, m, s, means != nullptr, stds != nullptr,
        reinterpret_cast<float4*>(out));
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_select_topk(const float* scores, int B, int A, const int32_t* candidates, int F, const int32_t* candidate_counts, int K,
                                const float* boxes, int64_t* sel_index, int32_t* sel_count, float* sel_scores, float* sel_boxes,
                                void* stream) {
    GNMS_CHECK_ARG(B >= 0 && A >= 0 && F >= 0 && K >= 0, "gnms_select_topk: negative size");
    if (B == 0 || K == 0) return GNMS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!candidates) F = A;
    if (A == 0 || F == 0) {
        if (sel_count) GNMS_CHECK_HIP(hipMemsetAsync(sel_count, 0, sizeof(int32_t) * B, st));
        if (sel_index) GNMS_CHECK_HIP(hipMemsetAsync(sel_index, 0xff, sizeof(int64_t) * (size_t)B * K, st));
        if (sel_scores) GNMS_CHECK_HIP(hipMemsetAsync(sel_scores, 0, sizeof(float) * (size_t)B * K, st));
        if (sel_boxes) GNMS_CHECK_HIP(hipMemsetAsync(sel_boxes, 0, sizeof(float) * 4 * (size_t)B * K, st));
        return GNMS_OK;
    }
    GNMS_CHECK_ARG(scores != nullptr, "gnms_select_topk: scores is NULL");
    // (every argument check sits in front of the stream-ordered temporary; the guard returns it to the pool on every later exit)
    GNMS_CHECK_ARG(!boxes || ((uintptr_t)boxes % 16 == 0), "gnms_select_topk: boxes must be 16-byte aligned");
    GNMS_CHECK_ARG(!sel_boxes || ((uintptr_t)sel_boxes % 16 == 0), "gnms_select_topk: sel_boxes must be 16-byte aligned");
    GNMS_CHECK_ARG(!sel_boxes || boxes, "gnms_select_topk: sel_boxes needs boxes");
    // several workgroups per image where one launch can hold them all (topk_coop_kernel): from 4096 candidates on
    {
        const int Kc = K < F ? K : F;
        const int G = std::max(gnms_div_up(F, kCoopChunk), gnms_div_up(Kc, 1024));
        // Its grid barriers need every workgroup resident at the same time.  B * G <= CUs is not enough when ANOTHER launch of the same kind runs
        // beside it on another stream (each could hold half the machine and wait for the rest for ever), so launches of this kernel are
        // chained across streams: one event per device, recorded behind every launch; a launch on a different stream than the last one waits
        // for it first (launches of one stream are ordered anyway).  (hipLaunchCooperativeKernel does the same job at +22 us of host time
        // per call -- measured.)  Not while the stream is being captured: the one-workgroup kernels below serve a capture.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        if (!capturing && F > 4096 && K <= GNMS_MAX_BOXES && (long)B * G <= (long)gnms_device_cu_count() && B <= kCoopMaxImages) {
            const int Kpad = gnms_div_up(Kc, 1024) * 1024;
            const size_t need = coop_scratch_bytes(B, G, Kpad);
            size_t lds = (size_t)gnms_div_up(Kc, 1024) * 1024 * 8;
            if (lds < kCoopBins * sizeof(unsigned)) lds = kCoopBins * sizeof(unsigned);
            int rc = gnms_allow_lds_raw(reinterpret_cast<const void*>(topk_coop_kernel), lds);
            if (rc) return rc;
            struct Chain { hipEvent_t ev = nullptr; hipStream_t last = nullptr; bool any = false; char* scratch = nullptr; size_t cap = 0; std::map<size_t, int> per_cu; };
            static std::mutex mu;
            static std::map<int, Chain> chains;
            int dev = 0;
            GNMS_CHECK_HIP(hipGetDevice(&dev));
            bool resident = true;
            {
                std::lock_guard<std::mutex> lock(mu);
                Chain& C = chains[dev];
                // residency as the runtime computes it for THIS kernel, workgroup size and LDS request (remembered per LDS size): the grid
                // barrier is only safe when occupancy x CUs covers the grid -- otherwise the one-workgroup kernels below
                auto it = C.per_cu.find(lds);
                if (it == C.per_cu.end()) {
                    int nb = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(topk_coop_kernel), 1024, lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
                    it = C.per_cu.emplace(lds, nb).first;
                }
                resident = (long)it->second * gnms_device_cu_count() >= (long)B * G;
            }
            if (resident) {
                std::lock_guard<std::mutex> lock(mu);
                Chain& C = chains[dev];
                if (!C.ev) GNMS_CHECK_HIP(hipEventCreateWithFlags(&C.ev, hipEventDisableTiming));
                if (need > C.cap) {                                    // (rare: the first call, or a bigger K; hipFree waits for the device)
                    if (C.scratch) GNMS_CHECK_HIP(hipFree(C.scratch));
                    C.scratch = nullptr; C.cap = 0;
                    const size_t cap = need + (need >> 1);
                    GNMS_CHECK_HIP(hipMalloc((void**)&C.scratch, cap));
                    GNMS_CHECK_HIP(hipMemset(C.scratch, 0, (size_t)kCoopMaxImages * sizeof(CoopScratch)));
                    C.cap = cap;
                }
                if (C.any && C.last != st) GNMS_CHECK_HIP(hipStreamWaitEvent(st, C.ev, 0));
                topk_coop_kernel<<<dim3(G, B), 1024, lds, st>>>(scores, A, candidates, F, candidate_counts, K, Kpad, G, C.scratch,
                                                                reinterpret_cast<const float4*>(boxes), (long long*)sel_index, sel_count, sel_scores,
                                                                reinterpret_cast<float4*>(sel_boxes));
                GNMS_CHECK_LAUNCH();
                GNMS_CHECK_HIP(hipEventRecord(C.ev, st));
                C.last = st;
                C.any = true;
                return GNMS_OK;
            }
        }
    }
    gnms_async_buffer pre_buf;                                        // [B][K] pre-selected candidates + [B] counts (large F only)
    if (F > GNMS_MAX_BOXES) {
        if (K > GNMS_MAX_BOXES) {
            gnms_set_error("gnms_select_topk: K=%d exceeds GNMS_MAX_BOXES=%d", K, GNMS_MAX_BOXES);
            return GNMS_ERR_UNSUPPORTED;
        }
        GNMS_CHECK_HIP(pre_buf.alloc(((size_t)B * K + B) * sizeof(int), st));
        int* pre = pre_buf.as<int>();
        topk_preselect_kernel<<<B, 1024, 0, st>>>(scores, A, candidates, F, candidate_counts, K, pre, pre + (size_t)B * K);
        GNMS_CHECK_LAUNCH();
        candidates = pre;
        candidate_counts = pre + (size_t)B * K;
        F = K;
    }
    const int P2 = next_pow2(F);
    const size_t lds = (size_t)P2 * 8;
    const int threads = P2 <= 1024 ? P2 : 1024;
#define GNMS_TOPK(EE)                                                                                                                  \
    do {                                                                                                                               \
        if (lds > 64 * 1024)                                                                                                           \
            GNMS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(select_topk_kernel<EE>),                                 \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                \
        select_topk_kernel<EE><<<B, threads, lds, st>>>(scores, A, candidates, F, candidate_counts, K, P2,                            \
                                                        reinterpret_cast<const float4*>(boxes), (long long*)sel_index, sel_count,      \
                                                        sel_scores, reinterpret_cast<float4*>(sel_boxes));                            \
    } while (0)
    switch (P2 <= 1024 ? 1 : P2 / 1024) {
        case 1: GNMS_TOPK(1); break;
        case 2: GNMS_TOPK(2); break;
        case 4: GNMS_TOPK(4); break;
        case 8: GNMS_TOPK(8); break;
        default: GNMS_TOPK(16); break;
    }
#undef GNMS_TOPK
    GNMS_CHECK_LAUNCH();
    GNMS_CHECK_HIP(pre_buf.release());
    return GNMS_OK;
}
