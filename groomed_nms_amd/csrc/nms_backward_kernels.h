// nms_backward_kernels.h -- backward of the GrooMeD-NMS layer (gfx950).
//
// The reference has no hand-written backward: autograd differentiates
//   prob = [threshold](clamp(M s, 0, 1))            lib/groomed_nms.py:111-127
// with M assembled from I - P (masked groups, :105), inverse(I_g + P_g) (:107) or inverse(I + P) (:110).
// Closed forms (restated in oracle/gnms_oracle.c):
//   gx_q   = dL/dprob routed to NMS position q, zeroed where the returned tensor was thresholded
//            in place (:115) or where the clamp saturated (torch.clamp passes the gradient AT the bounds)
//   masked : dL/ds_head = gx_head - sum_{i in group, i != head} P_i gx_i ; dL/ds_i = gx_i ;
//            dL/diou[i][head] = -gx_i s_head f'(iou[i][head])
// Everything is gather-form and deterministic (no float atomics): bit-identical run to run.
#pragma once
#include "nms_kernels.h"
#include "iou_grad.h"
#include "iou3d_grad.h"

namespace gnms {

// gx by NMS position.  One thread per returned element j.
__global__ __launch_bounds__(256) void bwd_gx_kernel(const float* __restrict__ grad_prob, int N, const int* __restrict__ counts,
                                                     gnms_params P, char* ws, gnms_ws_layout L) {
    const int b = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    if (j >= n) { I.gx[j] = 0.0f; return; }
    const int q = P.return_sorted_prob ? I.sidx[j] : j;              // prob[j] = r[sorted_indices[j]]  (:117)
    float g = grad_prob[(size_t)b * N + j];
    const float pre = I.pre[q];
    const float r2 = I.r2[q];
    const bool thresholded = P.return_sorted_prob || !P.group_boxes;  // which tensor was returned (:117,:124-127)
    if (thresholded && r2 < P.valid_box_prob_threshold) g = 0.0f;
    if (!(pre >= 0.0f && pre <= 1.0f)) g = 0.0f;
    I.gx[q] = g;
}

// masked groups, default path, ONE launch with two kinds of workgroups (hard sort, unsorted output: position q = rank):
//   blockIdx.x <  elem_blocks : one thread per rank: gx = dL/dprob where the clamp let it through; dL/ds = gx for every box
//                               in a group, 0 for boxes in no group -- except the heads of multi-member groups, which belong to
//   blockIdx.x >= elem_blocks : one WAVE per multi-member group (hlist): dL/ds_head = gx_head - sum_i P_i gx_i.  All lanes fetch
//                               the members' products in parallel (gx recomputed from dL/dprob, so the two kinds of workgroups
//                               do not depend on each other); the sum runs SEQUENTIALLY in member order (v_readlane + v_sub):
//                               deterministic and bit-identical to the left-to-right matmul row of the reference.
__device__ __forceinline__ float bwd_gx_of(const float* __restrict__ grad_prob_img, const ImgPtrs& I, int k) {
    const float pre = I.pre[k];
    return (pre >= 0.0f && pre <= 1.0f) ? grad_prob_img[k] : 0.0f;    // clamp passes the gradient at the bounds only
}

__global__ __launch_bounds__(256) void bwd_masked_fused_kernel(const float* __restrict__ grad_prob, int N, const int* __restrict__ counts,
                                                               gnms_params P, char* ws, gnms_ws_layout L, float* __restrict__ grad_scores,
                                                               int elem_blocks) {
    const int b = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    float* gs = grad_scores + (size_t)b * N;
    const float* gp = grad_prob + (size_t)b * N;
    if ((int)blockIdx.x >= elem_blocks) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int nheads = I.misc[1];
        const int nhb = (int)gridDim.x - elem_blocks;
        for (int hi = ((int)blockIdx.x - elem_blocks) * 4 + wave; hi < nheads; hi += nhb * 4) {
            const int k = I.hlist[hi];
            const int hstart = I.gstart[k], hlen = I.glen[k];
            float acc = bwd_gx_of(gp, I, k);
            for (int base = 1; base < hlen; base += 64) {
                const int t = base + lane;
                float prod = 0.0f;
                if (t < hlen) {
                    const int mk = I.gsorted[hstart + t];
                    prod = I.plead[mk] * bwd_gx_of(gp, I, mk);
                }
                const int cnt = min(64, hlen - base);
                for (int u = 0; u < cnt; ++u) acc -= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), u));
            }
            if (lane == 0) gs[I.order[k]] = acc;
        }
        return;
    }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    if (k >= n) { gs[k] = 0.0f; I.gx[k] = 0.0f; return; }
    const float g = bwd_gx_of(gp, I, k);
    I.gx[k] = g;
    const int h = I.head[k];
    if (h == k && I.glen[k] > 1 && I.misc[1] > 0) return;            // written by the head workgroups (hlist holds exactly these)
    gs[I.order[k]] = (h >= 0) ? g : 0.0f;
}

// The same result from the BACKWARD PLAN the forward's run builders leave (plan_entry, nms_kernels.h): one thread per plan position.
//   level 1: the plan entry (which rank sits here, where its gradient goes, its role);  level 2: pre, plead, dL/dprob of that rank, together.
// bwd_masked_fused_kernel's head waves go misc[1] -> hlist -> gstart / glen -> gsorted -> pre / plead / dL/dprob, five dependent round trips.
// A head's members are the FOLLOWING positions: their products come from the workgroup's LDS tile (256 positions + a halo of kPlanHalo, the
// halo's products computed once more by this workgroup), subtracted one after the other in member order exactly as the readlane loop does.
// The first 8 members per lane, every head of the wave at once; what a run has beyond them a wave takes 64 at a time.  A run longer than
// the halo (group_size > kPlanHalo) is walked by the wave that holds its head, plan entry by plan entry: today's loop, one level shorter.
// gx is stored only where bwd_masked_iou_kernel will read it (want_gx: dL/diou was asked for).
// Indices out of a plan are clamped to the image: a workspace the forward never filled yields garbage, not a wild access.
__device__ __forceinline__ void bwd_plan_terms(const float* __restrict__ gp, const ImgPtrs& I, int mk, float& g, float& prod) {
    const float pre = I.pre[mk], pl = I.plead[mk], d = gp[mk];
    g = (pre >= 0.0f && pre <= 1.0f) ? d : 0.0f;                     // (bwd_gx_of)
    prod = pl * g;
}

__global__ __launch_bounds__(256) void bwd_plan_kernel(const float* __restrict__ grad_prob, int N, char* ws, gnms_ws_layout L,
                                                       float* __restrict__ grad_scores, int want_gx) {
    __shared__ float prods[256 + kPlanHalo];
    const int b = blockIdx.y;
    ImgPtrs I = img_ptrs(ws, L, b);
    float* gs = grad_scores + (size_t)b * N;
    const float* gp = grad_prob + (size_t)b * N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = blockIdx.x * 256 + tid, ph = p + 256;
    const unsigned last = (unsigned)(N - 1);
    const bool halo = tid < kPlanHalo && ph < N;
    const u64 ent = p < N ? I.plan[p] : ((u64)kPlanPadBit << 32);
    const u64 eh = halo ? I.plan[ph] : 0ull;
    const unsigned lo = (unsigned)ent, hi = (unsigned)(ent >> 32);
    const int mk = (int)min(lo & 0x3fffu, last), dst = (int)min((lo >> 14) & 0x3fffu, last);
    const unsigned role = (hi >> 29) & 3u;
    const bool pad = (hi & kPlanPadBit) != 0u;
    float g = 0.0f, prod = 0.0f, gh, prodh = 0.0f;
    if (!pad && (role != kPlanZero || want_gx)) bwd_plan_terms(gp, I, mk, g, prod);
    if (halo && ((unsigned)(eh >> 61) & 3u) == kPlanMember) bwd_plan_terms(gp, I, (int)min((unsigned)eh & 0x3fffu, last), gh, prodh);
    prods[tid] = prod;
    if (tid < kPlanHalo) prods[256 + tid] = prodh;
    __syncthreads();
    // (no thread leaves here: the loops below are a whole wave's work, whichever lanes hold heads.  Positions >= N carry the padding role.)
    const bool live = p < N;
    if (live && want_gx) I.gx[pad ? p : mk] = g;                     // (padding entries carry g = 0)
    const bool head = role == kPlanHead;
    const int rlen = (int)((hi >> 14) & 0x7fffu);
    const int len = head ? min(rlen, kPlanHalo + 1) : rlen;
    float acc = g;
    if (head) {
        const float* m = prods + tid + 1;
#pragma unroll
        for (int u = 0; u < 8; ++u) { const float v = m[u]; if (u + 1 < len) acc -= v; }
    }
    // runs of more than 9: the wave takes them one at a time, 64 products per LDS read, the chain by v_readlane + v_sub
    u64 more = __ballot(head && len > 9);
    while (more) {
        const int src = __builtin_ctzll(more);
        more &= more - 1ull;
        const int hlen = __builtin_amdgcn_readlane(len, src), at = (tid & ~63) + src;
        float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), src));
        for (int base = 9; base < hlen; base += 64) {
            const int t = base + lane;
            const float v = t < hlen ? prods[at + t] : 0.0f;
            const int cnt = min(64, hlen - base);
            for (int u = 0; u < cnt; ++u) a -= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), u));
        }
        if (lane == src) acc = a;
    }
    // runs longer than the halo: their members' entries and terms from memory
    u64 longs = __ballot(role == kPlanLongHead);
    while (longs) {
        const int src = __builtin_ctzll(longs);
        longs &= longs - 1ull;
        const int hp = __builtin_amdgcn_readlane(p, src);
        const int hlen = min(__builtin_amdgcn_readlane(len, src), N - hp);
        float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), src));
        for (int base = 1; base < hlen; base += 64) {
            const int t = base + lane;
            float v = 0.0f, gm;
            if (t < hlen) bwd_plan_terms(gp, I, (int)min((unsigned)I.plan[hp + t] & 0x3fffu, last), gm, v);
            const int cnt = min(64, hlen - base);
            for (int u = 0; u < cnt; ++u) a -= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), u));
        }
        if (lane == src) acc = a;
    }
    if (live) gs[pad ? p : dst] = role == kPlanZero ? 0.0f : acc;
}

__global__ __launch_bounds__(256) void bwd_masked_kernel(int N, const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                                         float* __restrict__ grad_scores) {
    const int b = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    float* gs = grad_scores + (size_t)b * N;
    if (k >= n) { gs[k] = 0.0f; return; }
    const int c = I.order[k];
    gs[c] = (I.head[k] >= 0) ? I.gx[P.presorted ? c : k] : 0.0f;
}

// masked groups, part 2: one WAVE per multi-member group (hlist).  All lanes fetch the members' products P_i*gx_i in
// parallel (two memory round trips per 64 members); the head's value is then reduced SEQUENTIALLY in member order
// (v_readlane + v_sub, no memory on that path): deterministic, and bit-identical to the left-to-right accumulation of
// the reference's matmul row as restated by the oracle.
__global__ __launch_bounds__(256) void bwd_masked_heads_kernel(int N, gnms_params P, char* ws, gnms_ws_layout L, float* __restrict__ grad_scores) {
    const int b = blockIdx.y;
    ImgPtrs I = img_ptrs(ws, L, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nheads = I.misc[1];
    float* gs = grad_scores + (size_t)b * N;
    for (int hi = blockIdx.x * 4 + wave; hi < nheads; hi += gridDim.x * 4) {
        const int k = I.hlist[hi];
        const int hstart = I.gstart[k], hlen = I.glen[k];
        const int c = I.order[k];
        float acc = I.gx[P.presorted ? c : k];
        for (int base = 1; base < hlen; base += 64) {
            const int t = base + lane;
            float prod = 0.0f;
            if (t < hlen) {
                const int mk = I.gsorted[hstart + t];
                prod = I.plead[mk] * I.gx[P.presorted ? I.order[mk] : mk];
            }
            const int cnt = min(64, hlen - base);
            for (int u = 0; u < cnt; ++u) acc -= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), u));
        }
        if (lane == 0) gs[c] = acc;
    }
}

// sparse part of dL/diou for masked groups (the dense zero fill is a hipMemsetAsync before this kernel)
__global__ __launch_bounds__(256) void bwd_masked_iou_kernel(const float* __restrict__ iou, int N, long ld, const int* __restrict__ counts,
                                                             gnms_params P, char* ws, gnms_ws_layout L, float* __restrict__ grad_iou) {
    const int b = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    ImgPtrs I = img_ptrs(ws, L, b);
    const int h = I.head[k];
    if (h < 0 || h == k) return;
    const int ck = I.order[k], ch = I.order[h];
    if (P.presorted && !(ch < ck)) return;                           // entry killed by tril
    const int q = P.presorted ? ck : k;
    const size_t e = (size_t)b * N * ld + (size_t)ck * ld + ch;
    const float d = gnms_prune_grad(iou[e], P.nms_threshold, P.temperature, P.pruning_method);
    grad_iou[e] = (-(I.gx[q] * I.sscore[h])) * d;
}

// dL/d(geometry) of the masked-group layer (hard sort, unsorted output: bwd_masked_fused_kernel's / bwd_plan_kernel's modes) WITHOUT an
// N x N pass, for the 2D boxes behind gnms_forward_with_iou2d (MaskedBoxes) and the cuboids behind gnms_forward_with_iou3d
// (MaskedCuboids).  The layer's matrix gradient has one entry per non-head member k, at [member][head]
// (bwd_masked_iou_kernel), so
//   member k : dL/dbox_k    = g_k * d f(box_k, box_head)/da          one term, a plain store
//   head h   : dL/dbox_h    = sum_k g_k * d f(box_k, box_h)/db       sequentially in member order over the group's run
//   g_k = (-(gx_k s_h)) f'(q), q the matrix entry of (member, head) recomputed from the boxes as the forward computed it
// ONE launch with bwd_masked_fused_kernel's two kinds of workgroups: blockIdx.x < elem_blocks, one thread per rank (members; 0 for
// boxes in no group, heads without members and boxes behind counts[b]); above, one WAVE per multi-member group (hlist): the lanes fetch
// the members' terms in parallel, the G::kAcc sums then run SEQUENTIALLY in member order (v_readlane + v_add), as dL/ds_head does.
// The pair arithmetic is iou_grad.h's / iou3d_grad.h's, with the member as the row box, exactly as gnms_iou2d_backward /
// gnms_iou3d_backward<method 2> evaluates the same entry: a member's gradient is the same bits on both routes.  Indices out of the
// workspace are clamped to the image.
//
// A geometry G: kAcc sums and kFloats floats per box; Box, what a thread holds of an input row, and load(rows, index); Pair, pair(a, b)
// and add_grad(s, o, pair, g, acc) as the walker's (pair_grad_walker.h); entry(member, head, pair, P), the recomputed matrix entry;
// store(rows, out, index, acc), a finished sum to the output row, and store_zero(out, index) behind counts[b].
__device__ __forceinline__ float bwd_member_cotangent(const float* __restrict__ gp, const ImgPtrs& I, int k, int h, float q, const gnms_params& P) {
    const float d = gnms_prune_grad(q, P.nms_threshold, P.temperature, P.pruning_method);
    return (-(bwd_gx_of(gp, I, k) * I.sscore[h])) * d;
}

struct MaskedBoxes {
    static constexpr int kAcc = 4, kFloats = 4;
    struct Box {
        float4 b;
        float area;
    };
    using Pair = gnms_iou_grad::Pair;
    static __device__ __forceinline__ Box load(const float* __restrict__ rows, size_t i) {
        const float4 b = reinterpret_cast<const float4*>(rows)[i];
        return Box{b, gnms_iou_grad::box_area(b)};
    }
    static __device__ __forceinline__ Pair pair(const Box& a, const Box& b) { return gnms_iou_grad::pair_of(a.b, a.area, b.b, b.area); }
    static __device__ __forceinline__ float entry(const Box&, const Box&, const Pair& p, const gnms_params&) { return p.inter / p.uni; }
    static __device__ __forceinline__ void add_grad(const Box& s, const Box& o, const Pair& p, float g, float (&acc)[4]) {
        gnms_iou_grad::add_box_grad(s.b, o.b, p, g, acc);
    }
    static __device__ __forceinline__ void store(const float* __restrict__, float* __restrict__ out, size_t i, const float (&acc)[4]) {
        reinterpret_cast<float4*>(out)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    static __device__ __forceinline__ void store_zero(float* __restrict__ out, size_t i) {
        reinterpret_cast<float4*>(out)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
};

// A cuboid's record is rebuilt from its seven parameters (the forward's floats: corners_of + aabb_record), the matrix entry is the
// forward's own definition (nms_overlap3d_pair, guard band included).  Six extent sums per box, carried to the seven parameters ONCE
// per box (params_grad).
struct MaskedCuboids {
    static constexpr int kAcc = 6, kFloats = 7;
    struct Box {
        float4 u, v, e;                                               // the record, for the matrix entry
        gnms_iou3d_grad::Rec r;                                       // rec_of(u, v), for the gradient
    };
    using Pair = gnms_iou3d_grad::Pair;
    static __device__ __forceinline__ Box load(const float* __restrict__ rows, size_t i) {
        Box c;
        gnms_iou3d_grad::record_of_params(rows + i * 7, c.u, c.v, c.e);
        c.r = gnms_iou3d_grad::rec_of(c.u, c.v);
        return c;
    }
    static __device__ __forceinline__ Pair pair(const Box& a, const Box& b) { return gnms_iou3d_grad::pair_of(a.r, b.r); }
    static __device__ __forceinline__ float entry(const Box& member, const Box& head, const Pair&, const gnms_params& P) {
        return gnms_iou3d::nms_overlap3d_pair(member.u, member.v, member.e, head.u, head.v, head.e, P.nms_threshold);
    }
    static __device__ __forceinline__ void add_grad(const Box& s, const Box& o, const Pair& p, float g, float (&acc)[6]) {
        gnms_iou3d_grad::add_extent_grad<2>(s.r, o.r, p, g, acc);
    }
    static __device__ __forceinline__ void store(const float* __restrict__ rows, float* __restrict__ out, size_t i, const float (&acc)[6]) {
        float d[7];
        gnms_iou3d_grad::params_grad(rows + i * 7, acc, d);
#pragma unroll
        for (int c = 0; c < 7; ++c) out[i * 7 + c] = d[c];
    }
    static __device__ __forceinline__ void store_zero(float* __restrict__ out, size_t i) {
#pragma unroll
        for (int c = 0; c < 7; ++c) out[i * 7 + c] = 0.0f;
    }
};

template <class G>
__global__ __launch_bounds__(256) void bwd_masked_geometry_kernel(const float* __restrict__ grad_prob, const float* __restrict__ rows, int N,
                                                                  const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                                                  float* __restrict__ grad_rows, int elem_blocks) {
    using Box = typename G::Box;
    const int b = blockIdx.y;
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    const float* px = rows + (size_t)b * N * G::kFloats;
    float* gb = grad_rows + (size_t)b * N * G::kFloats;
    const float* gp = grad_prob + (size_t)b * N;
    const unsigned last = (unsigned)(n > 0 ? n - 1 : 0);
    if ((int)blockIdx.x >= elem_blocks) {
        if (n == 0) return;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int nheads = min(I.misc[1], n);
        const int nhb = (int)gridDim.x - elem_blocks;
        for (int hi = ((int)blockIdx.x - elem_blocks) * 4 + wave; hi < nheads; hi += nhb * 4) {
            const int k = (int)min((unsigned)I.hlist[hi], last);
            const int hstart = I.gstart[k], hlen = I.glen[k];
            if (hstart < 0 || hlen < 2 || hstart + hlen > n) continue;                    // (a workspace the forward never filled)
            const int ck = (int)min((unsigned)I.order[k], last);
            const Box hb = G::load(px, ck);
            float acc[G::kAcc];
#pragma unroll
            for (int c = 0; c < G::kAcc; ++c) acc[c] = 0.0f;
            for (int base = 1; base < hlen; base += 64) {
                const int t = base + lane;
                float term[G::kAcc];
#pragma unroll
                for (int c = 0; c < G::kAcc; ++c) term[c] = 0.0f;
                if (t < hlen) {
                    const int mk = (int)min((unsigned)I.gsorted[hstart + t], last);
                    const Box a = G::load(px, min((unsigned)I.order[mk], last));
                    const typename G::Pair p = G::pair(a, hb);
                    G::add_grad(hb, a, p, bwd_member_cotangent(gp, I, mk, k, G::entry(a, hb, p, P), P), term);
                }
                const int cnt = min(64, hlen - base);
                for (int u = 0; u < cnt; ++u) {
#pragma unroll
                    for (int c = 0; c < G::kAcc; ++c) acc[c] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term[c]), u));
                }
            }
            if (lane == 0) G::store(px, gb, ck, acc);
        }
        return;
    }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    if (k >= n) { G::store_zero(gb, k); return; }
    const int ck = (int)min((unsigned)I.order[k], last);
    const int h = I.head[k];
    if (h == k && I.glen[k] > 1 && I.misc[1] > 0) return;            // written by the head waves (hlist holds exactly these)
    float acc[G::kAcc];
#pragma unroll
    for (int c = 0; c < G::kAcc; ++c) acc[c] = 0.0f;
    if (h >= 0 && h != k && h < n) {
        const Box a = G::load(px, ck), hb = G::load(px, min((unsigned)I.order[h], last));
        const typename G::Pair p = G::pair(a, hb);
        G::add_grad(a, hb, p, bwd_member_cotangent(gp, I, k, h, G::entry(a, hb, p, P), P), acc);
    }
    G::store(px, gb, ck, acc);
}

}  // namespace gnms
