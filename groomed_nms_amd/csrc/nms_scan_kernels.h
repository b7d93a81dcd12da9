// nms_scan_kernels.h -- K3 of the GrooMeD-NMS layer: the leader scan (= the boxes classical greedy NMS keeps) on the threshold bit
// matrix W, as the general scan of one workgroup per image (leaders_body) and as the chain of one workgroup per super-block for a
// symmetric matrix (leaders_sb_body).  Shared by the layer (nms_kernels.h) and classic_nms.hip; the scan as a launch of its own,
// leaders_kernel, is in nms_leaders_kernel.h (nms_layer.hip and classic_nms.hip launch it, the tail units only use the bodies).
#pragma once
#include "gnms_device.h"

namespace gnms {
namespace {   // internal linkage: the header is included by several translation units

// ------------------------------------------------------------------------------------------------
// K3: leaders (= the boxes classical greedy NMS keeps).  The scan is inherently sequential over rank
// blocks; what must NOT be on that sequential path is global-memory latency.  Ranks are processed in
// super-blocks of kSB = 16 blocks (1024 ranks), software-pipelined inside ONE workgroup of 16 waves:
//   * removed-words of ALL blocks live in LDS (accAll[NB]);
//   * while wave 0 resolves super-block sb (registers + LDS only), waves 1..15 prefetch, for super-block
//     sb+1, the speculative triangular table  Xs[(b,b')][lane] = W[b'][rank(b,lane)]  (what each candidate
//     of block b would remove in blocks b' >= b of its own super-block): contiguous 512-B rows of W;
//   * the new leaders' words are PUSHED into the removed-words of all later blocks by gathering, per target block, exactly the
//     leaders' words (lane j = j-th leader of the super-block, from a list the resolve appends to): the 16 blocks of
//     super-block sb+1 by all waves right after the resolve ("near", one block per wave, the only part the next resolve
//     waits for), the blocks beyond by waves 1..15 WHILE wave 0 resolves sb+1 ("far").  B=8, N=4096: 28.6 -> 24.5 us.
// Resolve of one block: lane b' carries the removed-word of block b'; the 64 ranks are resolved on the
// scalar unit visiting only the leaders (s_ff1 on ~removed); each new leader ORs its table row into the
// lanes of the later blocks of the super-block.
// ------------------------------------------------------------------------------------------------
constexpr int kSB = 16;
constexpr int kSBPairs = kSB * (kSB + 1) / 2;
constexpr int kTabPer = (kSBPairs * 64 + 959) / 960;            // table entries per prefetching thread (waves 1..15)

#ifdef GNMS_TIMING   // developer instrumentation (tools/phase_ticks.py): s_memtime deltas of thread 0 (GNMS_RACC: thread 960) of image 0's workgroups
// accumulate in LDS -- round 5: a global read-modify-write per marker stalled wave 0 for a memory round trip, which the next barrier then
// waited for (every slot read ~1 us too long) -- and go to ws gx[] of image 0 once, at the end of the kernel (GNMS_TFLUSH)
__device__ __forceinline__ long long* gnms_tbuf() { __shared__ long long buf[32]; return buf; }
#define GNMS_TINIT() do { if (threadIdx.x < 32) gnms::gnms_tbuf()[threadIdx.x] = 0; __syncthreads(); } while (0)
#define GNMS_TFLUSH(ws_, L_, img_) do { __syncthreads(); if (threadIdx.x < 32 && (img_) == 0 && gnms::gnms_tbuf()[threadIdx.x]) \
        atomicAdd(reinterpret_cast<unsigned long long*>(gnms::img_ptrs(ws_, L_, 0).gx) + threadIdx.x, (unsigned long long)gnms::gnms_tbuf()[threadIdx.x]); } while (0)
#define GNMS_T0() long long t__ = (long long)__builtin_amdgcn_s_memtime()
#define GNMS_TACC(slot) do { long long n__ = (long long)__builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && b == 0) gnms::gnms_tbuf()[slot] += n__ - t__; t__ = n__; } while (0)   /* image 0's workgroup */
#define GNMS_TACC_IF(cond, slot) do { long long n__ = (long long)__builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && (cond)) gnms::gnms_tbuf()[slot] += n__ - t__; t__ = n__; } while (0)
#else
#define GNMS_TINIT() do {} while (0)
#define GNMS_TFLUSH(ws_, L_, img_) do {} while (0)
#define GNMS_TACC_IF(cond, slot) do {} while (0)
#define GNMS_T0() do {} while (0)
#define GNMS_TACC(slot) do {} while (0)
#endif

__device__ __forceinline__ int tri_index(int b, int bp) { return b * kSB - (b * (b - 1)) / 2 + (bp - b); }   // b <= bp < kSB

// exclusive OR-scan across the lanes of a wave
__device__ __forceinline__ u64 wave_or_exclusive_scan(u64 v, int lane) {
    u64 up = shfl_up_u64(v, 1);                                     // lane i <- lane i-1
    if (lane == 0) up = 0ull;
    return gnms_or_scan64(up);                                      // DPP inclusive OR-scan (gnms_common.h)
}

__host__ __device__ __forceinline__ size_t leaders_lds_layout(int NB, size_t* off_acc, size_t* off_lm, size_t* off_cand, size_t* off_pair) {
    size_t o = (size_t)kSBPairs * 64 * 8;                       // Xs
    *off_acc = o; o += (size_t)((NB + 1) & ~1) * 8;             // accAll[NB]
    *off_lm = o; o += (size_t)((NB + 1 + kSB) & ~1) * 8;        // leader masks of all blocks (+ kSB of padding the sym scan may read)
    *off_cand = o; o += 2 * (size_t)kSB * 64 * 4 + 128;        // leader ranks of the last two super-blocks + their counts (sym scan: list, claims, stamps)
    *off_pair = o; o += 2 * kSBPairs * 4;                       // pair -> (b, b')
    return o;
}

// dynamic LDS of leaders_kernel / leaders_body for an image of NB rank blocks (the one definition every launch site uses)
__host__ __device__ __forceinline__ size_t leaders_lds_size(int NB) {
    size_t a, l, c, p;
    return leaders_lds_layout(NB, &a, &l, &c, &p);
}

// epilogue of the leader scan, off the sequential path: leader lists, per-block words, running counts (lmask[nb] in LDS is final;
// `scratch` = >= (8 + nb) ints of LDS nobody else uses any more)
__device__ __forceinline__ void leaders_epilogue(const ImgPtrs& I, const u64* lmask, int nb, int* scratch) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // exclusive prefix of popcounts over blocks: thread i < nb owns block i (nb <= 256)
    int cnt = (tid < nb) ? __builtin_popcountll(lmask[tid]) : 0;
    const int inc = (int)gnms_add_scan32((unsigned)cnt);          // DPP prefix sum
    int* wsum = scratch;
    if (lane == 63 && wave < 4) wsum[wave] = inc;
    __syncthreads();
    int basew = 0;
    for (int w = 0; w < 4; ++w) if (w < wave) basew += wsum[w];
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    int* pfx = wsum + 8;                                          // [nb] exclusive prefix
    if (tid < nb) {
        pfx[tid] = basew + inc - cnt;
        I.leadw[tid] = lmask[tid];
        I.leadpfx[tid + 1] = basew + inc;
    }
    __syncthreads();
    for (int kb = wave; kb < nb; kb += 16) {
        const u64 mine = lmask[kb];
        if ((mine >> lane) & 1ull) {
            const int slot = pfx[kb] + __builtin_popcountll(mine & ((1ull << lane) - 1ull));
            const int k = (kb << 6) + lane;
            I.leadc[slot] = I.order[k];
            I.leadr[slot] = k;
        }
    }
    if (tid == 0) { I.misc[0] = total; I.leadpfx[0] = 0; }
}

// ------------------------------------------------------------------------------------------------
// K3 for a SYMMETRIC thresholded matrix whose rows W holds in full (from-boxes / from-records bit matrices; a matrix
// wsym_check_kernel passed) -- round 4: ONE WORKGROUP PER SUPER-BLOCK (16 blocks = 1024 ranks), the workgroups of an image on
// different CUs, handing the leader masks down the chain.
//
// What a super-block's leaders depend on is small -- the leader masks of the super-blocks before it, 128 bytes each -- and what
// turns those masks into "removed by an earlier leader" is large but has nothing sequential in it: rank (T, lane) overlaps a
// leader of source block bb iff  W[bb][rank] & mask[bb] != 0  (the matrix is symmetric), one coalesced 512-byte row segment per
// (source block, target block), 1 MiB per image at N = 4096, 16 MiB at 16384.  One workgroup per image pulled all of that through
// one CU's memory pipeline (~24 bytes per clock measured: 60k of the scan's 120k ticks on uniform boxes) between resolves that 15 of
// its 16 waves sat out.  Here workgroup j owns super-block j: it requests the row segments of source super-block s for its own 16
// blocks BEFORE the masks of s exist (the addresses do not depend on them), takes the masks when the workgroup of s publishes them,
// ANDs -- sources in ascending order, so the first hit of a rank is its claimer (rem[], what K4 used to compute) -- then resolves its
// own super-block, publishes, and stores rem[] for its ranks.  The chain is nsb hand-offs long; everything heavy runs beside it.
//
// HAND-OFF.  A mask travels as two 8-byte granules {epoch, 32 mask bits} written by single write-through stores and polled with
// agent-scope loads: a granule is valid iff its tag is the workspace's call counter (misc[8], advanced by the sort kernels of every
// call -- so stale granules of earlier calls, or of earlier replays of a captured graph, never match; the same kernels also zero the
// image's granules, so that whatever a recycled allocation held where they now lie cannot carry the tag by accident).
// No fence anywhere: beside the matrix writers one agent-scope release costs more than the whole scan (nms_writers.h).  rem[] goes
// out through write-through stores as well and is read back (groups_body / attribute_*) with agent-scope loads; the workgroup of the
// LAST super-block waits for the other workgroups' "rem stored" granules and carries on with K4..K6 of the image.
// A workgroup only ever waits for workgroups with a LOWER block index (dispatched before it).
//
// RESOLVE (inside a super-block).  The leaders are the unique solution of
//     L[r] = !ext[r]  &&  no q < r (same super-block) with L[q] and overlap(q, r).
// Wave tb owns block tb and iterates: from the current masks of the blocks before it (LDS, read at immediate offsets) and its table
// words t[bb] = W[kb0 + bb][rank (tb, lane)] (registers) it recomputes its own mask (the in-block fixed point of round 2), all 16
// waves at once, one LDS barrier per step, until a step changes no mask; a wave whose earlier blocks did not change since it last
// looked skips the step.  Block tb is exact after step tb + 1 at the latest, NMS inputs settle in 3-5 steps.  (What a step costs is
// LDS and VALU issue, 16 waves on 4 SIMDs: ~250 cycles for the barrier, ~500 for the 16 x 15 mask reads, ~1000 for the AND/ORs --
// tools/../build/mb/bar.hip -- so the parallel resolve is no faster than the scalar-unit resolve of round 2 per super-block; what it
// buys is that no wave idles and nothing else has to be overlapped with it.)
// ------------------------------------------------------------------------------------------------

// The super-blocks [j0, j1) of image `b`, one after the other (j1 <= nsb of the image; workgroup `me` of the image's `nwg` chain
// workgroups, which own contiguous ascending ranges -- so a workgroup only ever waits for workgroups with a lower index).  Returns true
// in the workgroup that may go on with K4..K6 of the image: the one whose range ends with the image's last super-block, after every
// rem[] entry of the image is visible to it.
//
// STAGE (round 5, the fast tail; STAGE = the overlap source, kFromMatrix / kFromBoxes / kFromRecords, or kNoStage): masked groups, hard sort.
// The workgroup that resolved a super-block knows, per rank k, the leader lr = rem[k] that took it -- and with it everything K5 computes for
// k as long as two things hold for the IMAGE: every leader is a member of its own group (overlap(L, L) > thr: any box of positive finite
// area), so head == leader, and no group is longer than the cap, so every member is kept.  It therefore evaluates
//     member = overlap(k, lr) > thr;  plead = prune(overlap);  pre = s_k - plead * s_lr  (s_k for a leader);  r2 = clamp(pre)
// right behind its resolve, for its own 1024 ranks, beside the chain (the masks are out by then), and stores head / plead / pre / r2
// write-through in front of its "rem stored" granule; a leader outside its own group raises the granule's `complex` bit.  The image's last
// workgroup then only has to check the two conditions (fast_final_body) before K6 -- no sort of the groups on the path to the
// probabilities -- and the groups' CSR the backward reads is built beside K6 by one more workgroup (csr_build_body).
// Returns 0 in the workgroups that are done, 1 in the image's last one (2: STAGE and some leader is outside its own group).
constexpr int kNoStage = -1;
constexpr int kFastGroupMax = 256;   // longest group the fast tail handles (default cap: 101)
constexpr int kGranVerdict = 30;     // gran[16][30]: the last workgroup's verdict for csr_build_body (payload 1 = fast tail, 2 = K5 ran, nothing to do)

// FUSED (round 6, one_launch_kernel; a single super-block: j0 = 0, j1 = 1): sort, bit table and this chain are workgroups of ONE launch.
// The sort's outputs are read with agent-scope loads (the caller has waited for the sort's flags); the super-block's table is not
// gathered from W but copied from the image the table workgroups leave where W lies (one_launch_bits_*: already in this layout, word
// (source block bb <= target block tb, target lane) = the bits M[target][source] -- the reference's own orientation, :250, so no
// symmetry is assumed and none is checked), behind a wait for their `nflags` flags; `tag` = the launch's call counter value.
template <int STAGE = kNoStage, bool FUSED = false>
__device__ __forceinline__ int leaders_sb_body(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, const int b, const int j0,
                                               const int j1, const int me, const float* __restrict__ stage_src = nullptr, long stage_ld = 0,
                                               const float stage_thr = 0.0f, const float stage_temp = 0.0f, const int stage_prune = 0,
                                               const int Ppow2 = 0, const unsigned tag = 0u, const int nflags = 0, const size_t lds_side = 0,
                                               const u64* __restrict__ ext0 = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    size_t oa, ol, oc, op;
    leaders_lds_layout(L.NB, &oa, &ol, &oc, &op);
    u64* Xs = reinterpret_cast<u64*>(smem);                      // [kSBPairs][64] table of the own super-block
    u64* lmask = reinterpret_cast<u64*>(smem + ol);              // [NB + kSB] leader masks: the earlier super-blocks' as they arrive, then the own
    int* pair_b = reinterpret_cast<int*>(smem + op);             // [kSBPairs]
    int* pair_bp = pair_b + kSBPairs;
    int* stamp = reinterpret_cast<int*>(smem + oc);              // [1] the last resolve step that changed a mask
    int* bstamp = stamp + 4;                                     // [kSB] per block of the super-block: the last step that changed its mask
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    // (the wave index through readfirstlane: as tid >> 6 it is a VECTOR value to the compiler, and every `bb < tb` below became a 64-bit
    // lane mask in an SGPR pair -- 186 spilled SGPRs and a v_readlane / s_nop pair around every use)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = (n + 63) >> 6;
    const int nsb = max(1, (nb + kSB - 1) / kSB);                  // (an EMPTY image still has one -- empty -- super-block: leaders_chain's count; its
                                                                   // workgroup must reach K4..K6, the only writers of the image's outputs)
    const u64 below = (1ull << lane) - 1ull;
    const bool last_wg = j1 == nsb;                                // this workgroup ends with the image's last super-block
    int have = 0;                                                  // super-blocks [0, have) have their masks in lmask (workgroup-uniform)
    int complex_img = 0;                                           // STAGE: a leader of this workgroup's ranks is outside its own group
    const u64 epoch = FUSED ? ((u64)tag << 32) : ((u64)(unsigned)I.misc[8] << 32);
    GNMS_T0();
    // table layout: pair (source block bb <= target block tb) at tb (tb + 1) / 2 + bb -- a target's words are consecutive, so the wave
    // that owns it reads them at immediate offsets from one base (the general scan's layout needs the triangular index per word:
    // ~12 scalar instructions each, and sixteen waves share the CU's one scalar unit)
    if (tid < kSB) for (int bb = 0; bb <= tid; ++bb) { pair_b[tid * (tid + 1) / 2 + bb] = bb; pair_bp[tid * (tid + 1) / 2 + bb] = tid; }
    for (int i = tid; i < nb + kSB; i += 1024) lmask[i] = 0ull;
    __syncthreads();
    for (int j = j0; j < j1; ++j) {
    const int kb0 = j * kSB;
    const int nblk = min(kSB, nb - kb0);
    const bool last_sb = j == nsb - 1;
    // STAGE: what the rank needs of itself (score, input index, box) is requested before anything is waited for
    float st_sk = 0.0f;
    int st_ck = 0;
    float4 st_bk = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (STAGE != kNoStage) {
        const int kk = ((kb0 + (wave < nblk ? wave : 0)) << 6) + lane;
        if constexpr (FUSED) {
            // the whole image's order / scores (/ boxes) by rank into LDS, beside everything else (smem + lds_side): the rank's own values and,
            // behind the resolve, its leader's come from there -- one gather level (the overlap entry) instead of two
            int* ordA = reinterpret_cast<int*>(smem + lds_side);
            float* sscA = reinterpret_cast<float*>(ordA + 1024);
            float4* rbxA = reinterpret_cast<float4*>(smem + lds_side + 8192);
            if (tid < n) {
                ordA[tid] = coh_load(I.order + tid);
                sscA[tid] = coh_load(I.sscore + tid);
                if (STAGE == kFromBoxes) rbxA[tid] = coh_load_f4(I.rbox + tid);
            }
        } else if (wave < nblk && kk < n) {
            st_sk = I.sscore[kk];
            st_ck = I.order[kk];
            if (STAGE == kFromBoxes) st_bk = I.rbox[kk];
        }
    }
    if (tid == 0) *stamp = 0;
    if (tid < kSB) bstamp[tid] = -1;
    {   // the own super-block's table: no dependence on anybody (in flight while the first masks are waited for)
        constexpr int kTabAll = (kSBPairs * 64 + 1023) / 1024;
        u64 tw[kTabAll];
        if constexpr (FUSED) {                                     // the table workgroups' flags, then their image of the table as it stands
            if (wave == 0) {
                for (int f0 = 0; f0 < nflags; f0 += 64) {         // (<= 13 x 32 flags: gran[3 .. 15])
                    const int f = f0 + lane < nflags ? f0 + lane : f0;
                    const u64 want = strong_gran(tag, kSlotBits + (unsigned)f);
                    const u64* g = I.gran + (size_t)3 * 32 + f;
                    while (__ballot(gran_load(g) != want) != 0ull) __builtin_amdgcn_s_sleep(1);
                }
            }
            __syncthreads();
            if constexpr (STAGE != kNoStage) {
                const int kk = ((kb0 + (wave < nblk ? wave : 0)) << 6) + lane;
                if (wave < nblk && kk < n) {
                    st_sk = reinterpret_cast<const float*>(smem + lds_side + 4096)[kk];
                    st_ck = reinterpret_cast<const int*>(smem + lds_side)[kk];
                    if (STAGE == kFromBoxes) st_bk = reinterpret_cast<const float4*>(smem + lds_side + 8192)[kk];
                }
            }
            const int npw = (nb * (nb + 1) / 2) * 64;              // the image's pairs (target block < nb): what the table workgroups wrote
#pragma unroll
            for (int u = 0; u < kTabAll; ++u) {
                const int e = tid + u * 1024;
                tw[u] = (e < npw) ? coh_load(I.W + e) : 0ull;
            }
        } else {
#pragma unroll
            for (int u = 0; u < kTabAll; ++u) {
                const int e = tid + u * 1024;
                tw[u] = 0ull;
                if (e < kSBPairs * 64) {
                    const int pr = e >> 6;
                    const int bb = pair_b[pr], bp = pair_bp[pr];
                    const int k = (kb0 + bp) * 64 + (e & 63);      // row block = the SOURCE block bb, column = target rank (bp, lane)
                    if (bp < nblk && k < n) tw[u] = I.W[(size_t)(kb0 + bb) * L.NC + k];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kTabAll; ++u) {
            const int e = tid + u * 1024;
            if (e < kSBPairs * 64) Xs[e] = tw[u];
        }
    }
    GNMS_TACC_IF(b == 0 && last_sb, 0);
    const int tb = wave;                                           // this wave's block of the super-block
    const bool live = tb < nblk;
    const int kT = ((kb0 + (live ? tb : 0)) << 6) + lane;          // this lane's rank
    lds_barrier();                                                 // the table is in LDS (and the previous super-block of this workgroup is done with it and the stamps)
    // ---- resolve of the own super-block: every wave its block, steps until no mask changes ----
#ifdef GNMS_TIMING
    long long r__ = (long long)__builtin_amdgcn_s_memtime();
#define GNMS_RACC(slot) do { long long n__ = (long long)__builtin_amdgcn_s_memtime(); if (threadIdx.x == 960 && b == 0 && last_sb) gnms_tbuf()[slot] += n__ - r__; r__ = n__; } while (0)
#else
#define GNMS_RACC(slot) do {} while (0)
#endif
    const int tbc = live ? tb : 0;
    const int k0 = (kb0 + tbc) << 6;
    u64 tailmask = 0ull;                                           // past the image's last rank: never leaders
    if (live) { const int nrows = min(64, n - k0); if (nrows < 64) tailmask = ~((1ull << nrows) - 1ull); }
    const u64* myX = Xs + (size_t)(tbc * (tbc + 1) / 2) * 64 + lane;   // this wave's table words: source block bb at myX[bb * 64]
    const u64* myL = lmask + kb0;                                  // (lmask is padded by kSB entries: no clamp)
    const u64 cs = live ? (myX[tbc * 64] & below) : 0ull;          // earlier ranks of the block that overlap rank k0 + lane
    unsigned tlo[kSB - 1], thi[kSB - 1];
#pragma unroll
    for (int bb = 0; bb < kSB - 1; ++bb) {                          // (entries past tb belong to other targets: masked)
        const u64 x = myX[bb * 64];
        tlo[bb] = (bb < tb) ? (unsigned)(x & 0xffffffffu) : 0u;
        thi[bb] = (bb < tb) ? (unsigned)(x >> 32) : 0u;
    }
    u64 mine = 0ull;                                               // this block's leader mask as last published (lmask[kb0 + tb])
    GNMS_RACC(21);
    // (Round 5 ran this fixed point SPECULATIVELY while the workgroup waits -- cold with no external removals, then warm after every source
    // ANDed in -- so that only a confirming step or two would be left behind the last source's masks.  Measured: no gain; on NMS inputs every
    // source removes ranks in all 16 blocks, the repair cascades through the blocks like a cold resolve (17 steps in all where there were 4,
    // the final call as long as before, the chain 10 k ticks longer).  One call, behind the last source.)
    u64 cur_prev = ~0ull;
    bool first = true;
    int looked = 0;                                                // the step of this wave's last look at the earlier masks
    int step = 1;
    auto resolve = [&](const u64 ext) {
        const u64 fixed = ext | tailmask;                          // never leaders: taken by earlier super-blocks, or past the image's last rank
        bool force = true;
        for (;;) {
            if (live) {                                            // (wave-uniform)
                // did a block before mine change since I last looked?  (lane bb holds block bb's stamp)
                const bool dirty = force || __ballot(lane < tb && bstamp[lane < kSB ? lane : 0] >= looked) != 0ull;
                if (dirty) {
                    looked = step;
                    unsigned vlo = 0u, vhi = 0u;
                    if (!first) {                                  // (the very first look finds every mask of the super-block still zero)
#pragma unroll
                        for (int bb = 0; bb < kSB - 1; ++bb) {      // (one batch of reads: behind a branch per group of blocks they serialise)
                            const u64 l = myL[bb];
                            vlo |= tlo[bb] & (unsigned)(l & 0xffffffffu);
                            vhi |= thi[bb] & (unsigned)(l >> 32);
                        }
                    }
                    const u64 cur = fixed | __ballot((vlo | vhi) != 0u);
                    GNMS_RACC(22);
                    if (first || cur != cur_prev) {                // (the same `cur` gives the same leaders)
                        cur_prev = cur;
                        u64 leaders = 0ull;
                        if (~cur != 0ull) {
                            const bool cand = ((cur >> lane) & 1ull) == 0ull;
                            leaders = ~cur;
                            for (;;) {                             // in-block fixed point: positions < t are final after t rounds
                                const u64 nl = __ballot(cand && (cs & leaders) == 0ull);
                                if (nl == leaders) break;
                                leaders = nl;
                            }
                        }
                        if (leaders != mine) {
                            mine = leaders;
                            if (lane == 0) { lmask[kb0 + tb] = leaders; bstamp[tb] = step; *stamp = step; }
                        }
                    }
                    first = false;
                    GNMS_RACC(23);
                }
            }
            force = false;
            lds_barrier();
            GNMS_RACC(24);
            const int last = *stamp;
            ++step;
            if (step - last > 1) break;                            // a whole step without a change (a faster wave may have stamped a later step: still <=)
        }
    };
    // ---- the earlier super-blocks, in ascending order: row segments requested, masks awaited, ANDed ----
    int cl = -1;                                                   // rank of the first leader (of an earlier super-block) that overlaps it
    for (int s = 0; s < j; ++s) {
        const int s0 = s * kSB;
        u64 wv[kSB];
#pragma unroll
        for (int bb = 0; bb < kSB; ++bb) wv[bb] = (live && kT < n) ? I.W[(size_t)(s0 + bb) * L.NC + kT] : 0ull;
        if (wave == 0 && s >= have) {                              // the masks of super-block s (another workgroup's, not seen yet): 32 granules, lane g polls granule g
            const u64* g = I.gran + (size_t)s * 32 + (lane & 31);
            u64 v = gran_load(g);
            while (__ballot((v & 0xffffffff00000000ull) != epoch) != 0ull) { __builtin_amdgcn_s_sleep(2); v = gran_load(g); }
            reinterpret_cast<unsigned*>(lmask + s0)[lane & 31] = (unsigned)(v & 0xffffffffu);   // (lanes 32..63 write the same words again)
        }
        lds_barrier();
        int c = -1;
#pragma unroll
        for (int bb = 0; bb < kSB; ++bb) {
            const u64 m = wv[bb] & lmask[s0 + bb];
            if (c < 0 && m != 0ull) c = ((s0 + bb) << 6) + __builtin_ctzll(m);
        }
        if (cl < 0) cl = c;
    }
    if (j + 1 > have) have = j + 1;                                // (every super-block up to j is in lmask from here on: polled above, or this workgroup's own)
    // (ext0, classical NMS in chunks -- classic_nms.hip: word kb of it = ranks of block kb that something OUTSIDE this scan has removed already)
    const u64 ext = __ballot(cl >= 0) | ((ext0 != nullptr && live) ? ext0[kb0 + tbc] : 0ull);   // removed-word of the wave's block (earlier super-blocks' leaders)
    GNMS_TACC_IF(b == 0 && last_sb, 1);
    if constexpr (FUSED) {
        // A single super-block with nobody to hand masks to: ONE wave walks the blocks in order -- lane = rank of the block, the table words of
        // block t2 against the masks of the blocks before it (wave-uniform: scalar registers), then the in-block fixed point -- no barrier and no
        // repeated steps: ~150-300 cycles per block where the sixteen-wave fixed point above takes 4-7 steps of ~1200 (N = 500: 4.3 -> ~1 us)
        if (wave == 0) {
            u64 m[kSB];
#pragma unroll
            for (int t2 = 0; t2 < kSB; ++t2) {
                m[t2] = 0ull;
                if (t2 < nblk) {                                   // (wave-uniform)
                    const u64* X = Xs + (size_t)(t2 * (t2 + 1) / 2) * 64 + lane;
                    u64 hit = 0ull;
#pragma unroll
                    for (int bb = 0; bb < t2; ++bb) hit |= X[bb * 64] & m[bb];
                    const u64 csq = X[t2 * 64] & below;
                    const int nr = min(64, n - ((kb0 + t2) << 6));
                    const u64 cur = __ballot(hit != 0ull) | (nr < 64 ? ~((1ull << nr) - 1ull) : 0ull);
                    u64 leaders = ~cur;
                    if (leaders != 0ull) {
                        const bool cand = ((cur >> lane) & 1ull) == 0ull;
                        for (;;) {                                 // in-block fixed point: positions < t are final after t rounds
                            const u64 nl = __ballot(cand && (csq & leaders) == 0ull);
                            if (nl == leaders) break;
                            leaders = nl;
                        }
                    }
                    m[t2] = leaders;
                    if (lane == 0) lmask[kb0 + t2] = leaders;
                }
            }
        }
        lds_barrier();
        mine = live ? lmask[kb0 + tb] : 0ull;
    } else {
        resolve(ext);
    }
#ifdef GNMS_TIMING
    if (threadIdx.x == 0 && b == 0 && last_sb) gnms_tbuf()[20] += step;
#endif
    // ---- publish the masks (the chain's critical path ends here), then rem[] ----
    if (!last_sb && wave == 0 && lane < 32) {
        const unsigned half = reinterpret_cast<const unsigned*>(lmask + kb0)[lane];
        gran_store(I.gran + (size_t)j * 32 + lane, epoch | half);
    }
    GNMS_TACC_IF(b == 0 && last_sb, 2);
    // rem[] of the wave's block: itself for a leader, else the first claimer -- an earlier super-block's (cl), else the first earlier
    // block of this super-block with a leader in the table word, else the own block
    {
        const int k = k0 + lane;
        int c = -1;
#pragma unroll
        for (int bb = 0; bb < kSB - 1; ++bb) {
            const u64 l = myL[bb];
            const unsigned mlo = tlo[bb] & (unsigned)(l & 0xffffffffu), mhi = thi[bb] & (unsigned)(l >> 32);
            if (c < 0 && (mlo | mhi) != 0u) c = ((kb0 + bb) << 6) + (mlo ? __builtin_ctz(mlo) : 32 + __builtin_ctz(mhi));
        }
        if (c < 0) { const u64 m = cs & mine; c = (m != 0ull) ? k0 + __builtin_ctzll(m) : k; }
        int r = k;
        if (((mine >> lane) & 1ull) == 0ull) r = ((ext >> lane) & 1ull) ? cl : c;
        if constexpr (STAGE != kNoStage) {
            // the last workgroup's last super-block stays in LDS for fast_final_body (the table is dead: every wave has passed a barrier behind
            // its last read of it): r2, head and input index by rank
            const bool park = last_wg && j == j1 - 1;
            float* r2L = reinterpret_cast<float*>(smem);                             // (finalize_fast_body's layout)
            int* hdL = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 4);
            int* ordL = reinterpret_cast<int*>(smem + (size_t)Ppow2 * 8);
            if (live && k < n) {
                const int lr = r;
                float sl = st_sk, ov;
                if (STAGE == kFromBoxes) {
                    float4 bl = st_bk;
                    if (lr != k) {
                        if constexpr (FUSED) { bl = reinterpret_cast<const float4*>(smem + lds_side + 8192)[lr]; sl = reinterpret_cast<const float*>(smem + lds_side + 4096)[lr]; }
                        else { bl = I.rbox[lr]; sl = I.sscore[lr]; }
                    }
                    ov = pair_iou(st_bk, bl);
                } else {
                    int cb = st_ck;
                    if (lr != k) {
                        if constexpr (FUSED) { cb = reinterpret_cast<const int*>(smem + lds_side)[lr]; sl = reinterpret_cast<const float*>(smem + lds_side + 4096)[lr]; }
                        else { cb = I.order[lr]; sl = I.sscore[lr]; }
                    }
                    ov = overlap_at<STAGE>(overlap_src<STAGE>(stage_src, I, b, N, stage_ld), stage_ld, st_ck, cb, stage_thr);
                }
                float pre = 0.0f, pl = 0.0f;
                int hd = -1;
                if (ov > stage_thr) {                              // strict > (:249)
                    hd = lr;
                    if (lr == k) pre = st_sk;
                    else { pl = gnms_prune(ov, stage_thr, stage_temp, stage_prune); pre = st_sk - pl * sl; }
                } else if (lr == k) complex_img = 1;               // a leader outside its own group (NaN / <= thr diagonal): K5 proper decides the heads
                const float r2 = pre < 0.0f ? 0.0f : (pre > 1.0f ? 1.0f : pre);      // torch.clamp keeps NaN
                if (park) { r2L[k] = r2; hdL[k] = hd; ordL[k] = st_ck; }
                rem_store(I.rem, k, r);
                rem_store(I.head, k, hd);
                __hip_atomic_store(I.plead + k, pl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(I.pre + k, pre, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(I.r2 + k, r2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (live && k < n) rem_store(I.rem, k, r);
        }
    }
    GNMS_TACC_IF(b == 0 && last_sb, 4);
    }   // super-blocks of this workgroup
    if (!last_wg) {
        // every wave waits for the acknowledgement of its OWN write-through stores (s_waitcnt vmcnt(0): the barrier alone is an
        // s_barrier, which orders nothing in memory -- ADVICE r4), then the barrier, then "rem stored" goes out
        __builtin_amdgcn_s_waitcnt(0x0f70);                        // vmcnt(0) (gfx9 encoding: vmcnt = bits 3:0 + 15:14; expcnt / lgkmcnt left at their maxima)
        const int cx = (STAGE != kNoStage) ? __syncthreads_or(complex_img) : (__syncthreads(), 0);
        if (tid == 0) gran_store(I.gran + (size_t)16 * 32 + me, epoch | 1ull | (cx ? 2ull : 0ull));
        return 0;
    }
    // ---- the image's last super-block: the other workgroups' rem[] must be there, then the per-image epilogue (all masks are in LDS) ----
    if (wave == 0 && me > 0) {
        const u64* g = I.gran + (size_t)16 * 32 + (lane < me ? lane : 0);
        u64 v = gran_load(g);
        while (__ballot((v & 0xffffffff00000000ull) != epoch) != 0ull) { __builtin_amdgcn_s_sleep(2); v = gran_load(g); }
        if (STAGE != kNoStage && __ballot((v & 2ull) != 0ull) != 0ull) complex_img = 1;
    }
    GNMS_TACC_IF(b == 0 && last_wg, 3);
    if constexpr (STAGE != kNoStage) {
        return __syncthreads_or(complex_img) ? 2 : 1;              // (leaders_epilogue: only the slow path needs the lists -- fast_final_body)
    } else {
        __syncthreads();
        leaders_epilogue(I, lmask, nb, reinterpret_cast<int*>(Xs));
        GNMS_TACC_IF(b == 0 && last_wg, 4);
        return 1;
    }
}

// The four per-image stages K3..K6 are written as device functions (`*_body`, 1024 threads, image index `b`) so that they
// run either as kernels of their own (thin wrappers below) or back to back inside ONE launch (tail_kernel).
// leaders_body: the GENERAL scan (matrix in, possibly asymmetric; classical NMS), one workgroup per image.  Table entry
// (b, b')[lane] = W[b'][rank(b, lane)], what candidate (b, lane) would remove in block b', pushed leader by leader; wave 0 resolves on
// the scalar unit (~130 cycles per leader) while waves 1..15 prefetch and push.  Symmetric matrices take leaders_sb_body above.
__device__ __forceinline__ void leaders_body(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, const int b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    size_t oa, ol, oc, op;
    leaders_lds_layout(L.NB, &oa, &ol, &oc, &op);
    u64* Xs = reinterpret_cast<u64*>(smem);                      // [kSBPairs][64]
    u64* accAll = reinterpret_cast<u64*>(smem + oa);             // [NB]
    u64* lmask = reinterpret_cast<u64*>(smem + ol);              // [NB]
    int* pair_b = reinterpret_cast<int*>(smem + op);             // [kSBPairs]
    int* pair_bp = pair_b + kSBPairs;
    int* llist = reinterpret_cast<int*>(smem + oc);              // [2][kSB * 64] ranks of the leaders of super-block sb (buffer sb & 1)
    int* lcount = llist + 2 * kSB * 64;                          // [2]
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = (n + 63) >> 6;
    const int nsb = (nb + kSB - 1) / kSB;
    GNMS_T0();
    if (tid < kSB) for (int bp = tid; bp < kSB; ++bp) { pair_b[tri_index(tid, bp)] = tid; pair_bp[tri_index(tid, bp)] = bp; }
    for (int i = tid; i < nb; i += 1024) { accAll[i] = 0ull; lmask[i] = 0ull; }
    __syncthreads();

    // table prefetch of super-block `sb` into registers, by the threads [first, 1024)
    u64 tw[kTabPer];
    auto table_load = [&](int sb, int first, int nthr) {
        const int kb0 = sb * kSB;
        const int nblk = min(kSB, nb - kb0);
#pragma unroll
        for (int u = 0; u < kTabPer; ++u) {
            const int e = (tid - first) + u * nthr;
            tw[u] = 0ull;
            if (tid >= first && e < kSBPairs * 64) {
                const int pr = e >> 6;
                const int bb = pair_b[pr], bp = pair_bp[pr];
                if (bp < nblk) {
                    // row block = the target block bp, column = candidate rank (bb, lane): contiguous 512 B per (b, b') row
                    const int k = (kb0 + bb) * 64 + (e & 63);
                    if (k < n) tw[u] = I.W[(size_t)(kb0 + bp) * L.NC + k];
                }
            }
        }
    };
    auto table_store = [&](int first, int nthr) {
#pragma unroll
        for (int u = 0; u < kTabPer; ++u) {
            const int e = (tid - first) + u * nthr;
            if (tid >= first && e < kSBPairs * 64) Xs[e] = tw[u];
        }
    };
    // prologue: table of super-block 0 (waves 1..15 so the register footprint is the same as in the loop)
    table_load(0, 64, 960);
    table_store(64, 960);
    __syncthreads();
    GNMS_TACC(0);

    // push: OR the words of super-block `src`'s leaders into the removed-words of the blocks [first, last); the calling waves are
    // numbered w of nw and take every nw-th block, four blocks at a time.  Lane j gathers the word of the j-th leader (the resolve
    // appends every leader to a list as it finds it) -- exactly the words that matter, and all of a wave's blocks in ONE memory
    // round trip.
    auto push = [&](int src, int first, int last, int w, int nw) {
        const int* list = llist + (src & 1) * (kSB * 64);
        const int nl = lcount[src & 1];
        for (int base = first + w; base < last; base += 4 * nw) {
            u64 a[4] = {0ull, 0ull, 0ull, 0ull};
            for (int j0 = 0; j0 < nl; j0 += 64) {
                const int j = j0 + lane;
                const int lr = (j < nl) ? list[j] : -1;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kbp = base + u * nw;
                    if (lr >= 0 && kbp < last) a[u] |= I.W[(size_t)kbp * L.NC + lr];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kbp = base + u * nw;
                if (kbp < last) {                                  // wave-uniform
                    const u64 acc = gnms_wave_or(a[u]);
                    if (lane == 0 && acc != 0ull) atomicOr(reinterpret_cast<unsigned long long*>(&accAll[kbp]), (unsigned long long)acc);
                }
            }
        }
    };

    // Per super-block sb:  wave 0 resolves it (registers and LDS only) WHILE waves 1..15 prefetch the table of sb+1 and push the
    // leaders of sb-1 into the blocks from super-block sb+1 on ("far" push: nothing the running resolve reads);  then all 16 waves
    // push the new leaders of sb into the 16 blocks of super-block sb+1 ("near" push, one block per wave), the only part of the
    // push the next resolve has to wait for.
    for (int sb = 0; sb < nsb; ++sb) {
        const int kb0 = sb * kSB;
        const int nblk = min(kSB, nb - kb0);
        if (wave != 0) {
            if (sb + 1 < nsb) table_load(sb + 1, 64, 960);
            if (sb >= 1) push(sb - 1, (sb + 1) * kSB, nb, wave - 1, 15);
        } else {
            // ---- sequential resolve of this super-block: registers and LDS only ----
            u64 myacc = (lane < nblk) ? accAll[kb0 + lane] : 0ull;     // lane b' = removed-word of block kb0+b'
            u64 mylead = 0;                                            // lane b' = leader mask of block kb0+b'
            int* list = llist + (sb & 1) * (kSB * 64);
            int filled = 0;                                            // leaders of this super-block so far (wave-uniform)
            for (int bb = 0; bb < nblk; ++bb) {
                const int k0 = (kb0 + bb) << 6;
                const int nrows = min(64, n - k0);
                u64 cur = readlane64(myacc, bb);
                if (nrows < 64) cur |= ~((1ull << nrows) - 1ull);     // ranks >= n never lead
                if (~cur == 0ull) continue;                            // everything in this block is already removed
                const u64 d = Xs[tri_index(bb, bb) * 64 + lane];       // what rank k0+lane removes inside its own block
                // lane b' (> bb) also ORs the table row of every new leader into its removed-word; the LDS read of
                // leader i is consumed one trip later, so its latency hides behind the scalar chain of leader i+1
                const bool tgt = lane > bb && lane < nblk;
                const u64* row = Xs + (size_t)tri_index(bb, tgt ? lane : bb) * 64;
                u64 leaders = 0, pend = 0;
                do {                                                   // scalar loop: one trip per leader
                    const int p = __builtin_ctzll(~cur);
                    leaders |= 1ull << p;
                    const u64 nxt = row[p];
                    cur |= readlane64(d, p) | (1ull << p);             // a leader always leaves `remaining`
                    myacc |= tgt ? pend : 0ull;
                    pend = nxt;
                } while (~cur != 0ull);
                myacc |= tgt ? pend : 0ull;
                if (lane == bb) mylead = leaders;
                // the block's leaders join the list the pushes gather by (`leaders` is wave-uniform: one masked LDS store)
                if ((leaders >> lane) & 1ull) list[filled + __builtin_popcountll(leaders & ((1ull << lane) - 1ull))] = k0 + lane;
                filled += __builtin_popcountll(leaders);
            }
            if (lane < nblk) lmask[kb0 + lane] = mylead;
            if (lane == 0) lcount[sb & 1] = filled;
        }
        GNMS_TACC(1);
        __syncthreads();                                               // (A) wave 0 is done with Xs; the far pushes have landed
        GNMS_TACC(2);
        push(sb, kb0 + nblk, min(kb0 + nblk + kSB, nb), wave, 16);
        if (sb + 1 < nsb) table_store(64, 960);                        // land the prefetched table for the next super-block
        GNMS_TACC(3);
        __syncthreads();                                               // (B)
        GNMS_TACC(4);
    }
    leaders_epilogue(I, lmask, nb, reinterpret_cast<int*>(Xs));
}

// One CHAIN workgroup of a launch that runs the leader scan of B images with `spw` workgroups per image (spw = ceil(NB / 16) when the
// launch may meet symmetric images -- leaders_chain_wgs --, else 1); chain index c = (workgroup of the image) * B + image, so that the
// workgroups of the first super-blocks, which wait for nobody, are dispatched first.  sym_arg: 0 general, 1 symmetric (W holds full
// rows), 2 as wsym_check_kernel found this image's matrix.  Returns true, with *image set, in the ONE workgroup per image that goes
// on with K4..K6.
// workgroups per image: one per super-block, at most `cap` (0: no cap).  The launches that run beside a matrix write of their own
// (large images) cap it so that the chain leaves the writers their CUs.
__host__ __device__ inline int leaders_chain_wgs(int N, int sym_arg, int cap = 0) {
    const int nsb = max(1, ((N + 63) / 64 + kSB - 1) / kSB);
    const int w = sym_arg ? nsb : 1;
    return (cap > 0 && w > cap) ? cap : w;
}

// Returns 0 in the workgroups that are done; in the ONE workgroup per image that goes on with K4..K6: 1 (symmetric scan; with STAGE the
// fast tail's values are stored, see leaders_sb_body), 2 (the same, but some leader is outside its own group), 3 (general scan).
template <int STAGE = kNoStage>
__device__ __forceinline__ int leaders_chain(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, const int B, const int spw,
                                             const int c, const int sym_arg, int* image, const float* __restrict__ stage_src = nullptr,
                                             long stage_ld = 0, const float stage_thr = 0.0f, const float stage_temp = 0.0f,
                                             const int stage_prune = 0, const int Ppow2 = 0, const u64* __restrict__ ext0 = nullptr) {
    const int jw = c / B, b = c - jw * B;
    *image = b;
    // sym_arg: 0 general, 1 symmetric, 2 as wsym_check_kernel found, 3 symmetric on trust (the check runs in this launch: wsym_check_in_launch)
    const int sym = sym_arg == 2 ? (img_ptrs(ws, L, b).misc[3] == 0 ? 1 : 0) : (sym_arg == 3 ? (img_ptrs(ws, L, b).misc[2] == 0 ? 1 : 0) : sym_arg);
    if (!sym) {
        if (jw != spw - 1) return 0;
        leaders_body(N, counts, ws, L, b);
        return 3;
    }
    // symmetric: the image's own super-blocks (ragged counts: fewer than the launch provides for) in contiguous ranges of q
    const int n = gnms_count(counts, b, N);
    const int nsb = max(1, (((n + 63) >> 6) + kSB - 1) / kSB);
    const int q = (nsb + spw - 1) / spw;
    const int j0 = jw * q, j1 = min(nsb, j0 + q);
    if (j0 >= j1) return 0;                                        // (workgroup-uniform)
    return leaders_sb_body<STAGE>(N, counts, ws, L, b, j0, j1, jw, stage_src, stage_ld, stage_thr, stage_temp, stage_prune, Ppow2, 0u, 0, 0, ext0);
}

}  // namespace
}  // namespace gnms
