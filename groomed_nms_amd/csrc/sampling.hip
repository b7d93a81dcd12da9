// sampling.hip -- hard-anchor sampling, the sample weights and the weighted classification term of the reference's RPN loss
// (lib/loss/rpn_3d.py:458-472, 583-612, 885-1001) on the device, for B images at once.  DESIGN.md 3.14.
//
// gnms_sample_anchors: six stream-ordered launches, no global atomics, no inter-workgroup waits, no allocation.  A workgroup owns
// SMP_SPAN consecutive anchors of one image; what a launch hands to the next goes through per-workgroup slots in the caller's
// workspace, written with plain stores (as targets.hip does), and every workgroup of the next launch merges the slots of its image
// itself (the same sums in the same order everywhere: the result does not depend on which workgroup runs when).
//   sample_hist<0>     per workgroup: n_fg, n_bg and, per class, the histogram of bits 31..24 of the ordered key
//   sample_hist<1..3>  merge the previous level (level 0: also the quotas, :583-588) -> the digit that holds the k-th smallest key and
//                      what remains of k; histogram of the next 8 bits over the keys that share the prefix
//   sample_count       merge level 3 -> the cut value T and e = how many of the anchors equal to it are taken; per workgroup the
//                      foreground below T, the foreground at T and the background at T
//   sample_mark        prefix over the preceding workgroups' counts, then the span in anchor order: an anchor is sampled when its key is
//                      below T, or equals T and fewer than e equal anchors precede it in the image (ties: the lower index first);
//                      labels, bbox_weights, labels_scores, the sampled class, and the sampled foreground compacted in ascending order
// A class that is not cut (quota 0 or quota == members, :591 / :597) is taken whole: no histogram, no key compared.
// Every kernel loads its span's targets first and then its scores (load_span): two waits for memory per lane instead of two per tile.
//
// gnms_cls_loss: two launches.  cls_loss_main: one lane per anchor, the weight in float64 rounded once (:913-971), log-softmax cross
// entropy in float32 (subtract the row maximum, log of the sum of exps), the clamp, the un-normalised gradient, and per workgroup the
// float64 sum, the active count and the accuracy counts in slots; cls_loss_finish: merges the slots, writes the scalars and scales
// the gradient by cls_2d_lambda / active.
#include <math.h>
#include "gnms_common.h"

namespace {

constexpr int SMP_THREADS = 256;
constexpr int SMP_WAVES = SMP_THREADS / GNMS_WAVE;
constexpr int SMP_TILES = 8;                          // consecutive tiles of SMP_THREADS anchors per workgroup of the sampler
constexpr int SMP_SPAN = SMP_THREADS * SMP_TILES;
constexpr int CLS_TILES = 1;                          // the same for cls_loss_main (one tile: ~4 resident workgroups per CU hide the row's dependent loads)
constexpr int CLS_SPAN = SMP_THREADS * CLS_TILES;
constexpr int FIN_ELEMS = 16;                         // gradient entries per lane of cls_loss_finish
constexpr int SMP_IGN = 3000;                         // IGN_FLAG (:184)
constexpr int KIND_IGN = 0, KIND_FG = 1, KIND_BG = 2, KIND_NONE = 3;   // NONE: label 0, never sampled (skipped image, NaN target)

struct SelState {        // per (level, image, class)
    unsigned cut;        // the quota cuts this class
    unsigned prefix;     // the digits of the cut value found so far, right-aligned
    unsigned krem;       // the k-th smallest among the keys that share the prefix is the cut value
    unsigned take;       // anchors of the class that end up sampled
};
struct ImgInfo { int n_fg, n_bg, fg_num, bg_num; };

struct SmpArgs {
    const float* tl;            // [B][R] with stride ld_tl between anchors
    long long ld_tl;
    const float* prob;          // [B][R][C]
    const unsigned char* skip;  // [B] or null
    int B, R, C, nwg;
    double box_samples, fg_fraction;
    long long* labels;
    float* bbox_weights;
    float* labels_scores;
    unsigned char* sampled;
    int32_t* fg_index;
    int32_t* fg_counts;
    int32_t* counts;            // [B][6]
    // workspace
    unsigned* hist;             // [2][B][nwg][2][256]
    int* cnt0;                  // [B][nwg][2]   n_fg, n_bg of the workgroup
    int* cnt1;                  // [B][nwg][4]   fg below T, fg at T, bg at T
    SelState* state;            // [4][B][2]
    ImgInfo* info;              // [B]
};

// float -> uint32, ascending, -0 == +0, every NaN above +inf (np.argsort puts NaN last)
__device__ __forceinline__ unsigned okey32(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

struct Item { int kind, label; unsigned key; float score; };

// :458-472.  A target above zero that is no class index in [1, C) counts as ignore (the reference would index prob out of range)
__device__ __forceinline__ void decode_target(float t, int C, int& kind, int& label) {
    kind = KIND_NONE; label = 0;
    if (t > 0.0f) {
        const int l = t < 2147483520.0f ? (int)t : 0x7fffffff;
        if (l >= 1 && l < C) { kind = KIND_FG; label = l; }
        else kind = KIND_IGN;
    } else if (t < 0.0f) {
        kind = KIND_BG;
    } else if (t == 0.0f) {
        kind = KIND_IGN;
    }
}

// The workgroup's span, anchor blockIdx.x * SMP_SPAN + k * SMP_THREADS + threadIdx.x in it[k]: all targets are loaded first, then all
// scores (the sort keys of :592 / :598), so a lane waits for memory twice and not twice per tile.  A score is loaded for the foreground
// when want_fg, for the background when want_bg, for label-0 anchors outside both when want_rest; anchors past R and anchors of a
// skipped image come back as KIND_NONE with score 0.
__device__ __forceinline__ void load_span(const SmpArgs& a, int b, bool skipped, bool want_fg, bool want_bg, bool want_rest,
                                          Item (&it)[SMP_TILES]) {
    float t[SMP_TILES];
    const int r_first = blockIdx.x * SMP_SPAN + threadIdx.x;
    const long long row0 = (long long)b * a.R;
#pragma unroll
    for (int k = 0; k < SMP_TILES; ++k) {
        const int r = r_first + k * SMP_THREADS;
        t[k] = (!skipped && r < a.R) ? a.tl[(row0 + r) * a.ld_tl] : __uint_as_float(0x7fc00000u);
    }
#pragma unroll
    for (int k = 0; k < SMP_TILES; ++k) {
        const int r = r_first + k * SMP_THREADS;
        decode_target(t[k], a.C, it[k].kind, it[k].label);
        const bool in = !skipped && r < a.R;
        const bool want = in && ((it[k].kind == KIND_FG && want_fg) || (it[k].kind == KIND_BG && want_bg) || (it[k].kind == KIND_NONE && want_rest));
        it[k].score = want ? a.prob[(row0 + r) * a.C + it[k].label] : 0.0f;
        it[k].key = okey32(it[k].score);
    }
}

__device__ __forceinline__ int block_sum(int v, int* red) {
    const int lane = threadIdx.x & (GNMS_WAVE - 1), wave = threadIdx.x / GNMS_WAVE;
    const unsigned s = gnms_add_scan32((unsigned)v);
    __syncthreads();                                       // red may still be read from the previous use
    if (lane == GNMS_WAVE - 1) red[wave] = (int)s;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) t += red[w];
    return t;
}

// exclusive prefix sum over the workgroup's lanes in thread order; total = the sum of all
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, int* red, unsigned& total) {
    const int lane = threadIdx.x & (GNMS_WAVE - 1), wave = threadIdx.x / GNMS_WAVE;
    const unsigned s = gnms_add_scan32(v);
    __syncthreads();
    if (lane == GNMS_WAVE - 1) red[wave] = (int)s;
    __syncthreads();
    unsigned before = 0, t = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) {
        const unsigned x = (unsigned)red[w];
        if (w < wave) before += x;
        t += x;
    }
    total = t;
    return before + s - v;
}

__device__ __forceinline__ bool image_skipped(const SmpArgs& a, int b) { return a.skip && a.skip[b] != 0; }

// :583-588 with Python's round (half to even, on float64)
__device__ __forceinline__ void quotas(const SmpArgs& a, int n_fg, int n_bg, int& fg_num, int& bg_num) {
    if (isinf(a.box_samples)) { fg_num = n_fg; bg_num = n_bg; return; }
    const double all = (double)a.R * a.box_samples;
    const double qf = fmin(rint(all * a.fg_fraction), (double)n_fg);
    fg_num = (int)qf;
    const double qb = fmin(rint(all - (double)fg_num), (double)n_bg);
    bg_num = (int)qb;
}

// The digit of level `level` of both classes' cut values, from the workgroups' histograms of that level; every workgroup of the image
// computes the same.  prev: the state before the level (level 0: made here from the counts).  lds: 2 ints per class.
__device__ void resolve_level(const SmpArgs& a, int b, int level, SelState* cur, ImgInfo* info_out, int* red, unsigned* lds) {
    SelState st[2];
    if (level == 0) {
        int f = 0, g = 0;
        for (int w = threadIdx.x; w < a.nwg; w += SMP_THREADS) {
            f += a.cnt0[((long long)b * a.nwg + w) * 2 + 0];
            g += a.cnt0[((long long)b * a.nwg + w) * 2 + 1];
        }
        const int n_fg = block_sum(f, red), n_bg = block_sum(g, red);
        int fg_num, bg_num;
        quotas(a, n_fg, n_bg, fg_num, bg_num);
        st[0].cut = fg_num > 0 && fg_num != n_fg;            // :591
        st[1].cut = bg_num > 0 && bg_num != n_bg;            // :597
        st[0].prefix = st[1].prefix = 0u;
        st[0].krem = (unsigned)fg_num; st[1].krem = (unsigned)bg_num;
        st[0].take = st[0].cut ? (unsigned)fg_num : (unsigned)n_fg;
        st[1].take = st[1].cut ? (unsigned)bg_num : (unsigned)n_bg;
        info_out->n_fg = n_fg; info_out->n_bg = n_bg; info_out->fg_num = fg_num; info_out->bg_num = bg_num;
    } else {
        const SelState* prev = a.state + ((long long)(level - 1) * a.B + b) * 2;
        st[0] = prev[0]; st[1] = prev[1];
    }
    const unsigned* hist = a.hist + (size_t)(level & 1) * a.B * a.nwg * 512;
    for (int c = 0; c < 2; ++c) {
        if (!st[c].cut) continue;                            // uniform
        unsigned h = 0;
#pragma unroll 8
        for (int w = 0; w < a.nwg; ++w) h += hist[(((long long)b * a.nwg + w) * 2 + c) * 256 + threadIdx.x];
        unsigned total;
        const unsigned excl = block_excl_scan(h, red, total);
        if (threadIdx.x == 0) { lds[2 * c] = 255u; lds[2 * c + 1] = 1u; }     // (never kept: 1 <= krem <= total)
        __syncthreads();
        if (excl < st[c].krem && st[c].krem <= excl + h) { lds[2 * c] = threadIdx.x; lds[2 * c + 1] = st[c].krem - excl; }
        __syncthreads();
        st[c].prefix = (st[c].prefix << 8) | lds[2 * c];
        st[c].krem = lds[2 * c + 1];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        SelState* out = a.state + ((long long)level * a.B + b) * 2;
        out[0] = st[0]; out[1] = st[1];
    }
    cur[0] = st[0]; cur[1] = st[1];
}

// one more of digit d of class c: lanes of a wave that share a digit add once (probabilities crowd into a few exponent digits)
__device__ __forceinline__ void hist_add(unsigned* h, bool m, unsigned d) {
    const int lane = threadIdx.x & (GNMS_WAVE - 1);
    unsigned long long act = __ballot(m);
    for (int it = 0; it < 3 && act; ++it) {                  // uniform
        const int leader = __ffsll((long long)act) - 1;
        const unsigned d0 = (unsigned)__shfl((int)d, leader);
        const unsigned long long same = __ballot(m && d == d0);
        if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
        if (m && d == d0) m = false;
        act &= ~same;
    }
    if (m) atomicAdd(&h[d], 1u);
}

template <int LEVEL>
__global__ __launch_bounds__(SMP_THREADS) void sample_hist(SmpArgs a) {
    __shared__ unsigned h[2][256];
    __shared__ int red[SMP_WAVES];
    __shared__ unsigned dl[4];
    const int b = blockIdx.y;
    SelState st[2];
    if (LEVEL > 0) {
        ImgInfo info;
        resolve_level(a, b, LEVEL - 1, st, &info, red, dl);
        if (LEVEL == 1 && blockIdx.x == 0 && threadIdx.x == 0) a.info[b] = info;
    }
    h[0][threadIdx.x] = 0u;
    h[1][threadIdx.x] = 0u;
    __syncthreads();
    const bool skipped = image_skipped(a, b);
    int n_fg = 0, n_bg = 0;
    constexpr int SHIFT = 24 - 8 * LEVEL;
    constexpr int PSHIFT = LEVEL == 0 ? 0 : SHIFT + 8;        // the digits above this level's
    if (LEVEL == 0 || st[0].cut || st[1].cut) {               // uniform
        Item items[SMP_TILES];
        load_span(a, b, skipped, LEVEL == 0 || st[0].cut, LEVEL == 0 || st[1].cut, false, items);
#pragma unroll
        for (int tile = 0; tile < SMP_TILES; ++tile) {
            if (blockIdx.x * SMP_SPAN + tile * SMP_THREADS >= a.R) break;     // uniform
            const Item it = items[tile];
            const unsigned d = (it.key >> SHIFT) & 255u;
            bool mf = it.kind == KIND_FG, mb = it.kind == KIND_BG;
            if (LEVEL == 0) {
                n_fg += mf; n_bg += mb;
            } else {
                mf = mf && st[0].cut && (it.key >> PSHIFT) == st[0].prefix;
                mb = mb && st[1].cut && (it.key >> PSHIFT) == st[1].prefix;
            }
            hist_add(h[0], mf, d);
            hist_add(h[1], mb, d);
        }
    }
    __syncthreads();
    unsigned* out = a.hist + (size_t)(LEVEL & 1) * a.B * a.nwg * 512 + ((long long)b * a.nwg + blockIdx.x) * 512;
    out[threadIdx.x] = h[0][threadIdx.x];
    out[256 + threadIdx.x] = h[1][threadIdx.x];
    if (LEVEL == 0) {
        const int f = block_sum(n_fg, red), g = block_sum(n_bg, red);
        if (threadIdx.x == 0) {
            a.cnt0[((long long)b * a.nwg + blockIdx.x) * 2 + 0] = f;
            a.cnt0[((long long)b * a.nwg + blockIdx.x) * 2 + 1] = g;
        }
    }
}

// the cut value and the number of equal keys taken, from the state after level 3
__device__ __forceinline__ void cut_of(const SelState& s, unsigned& T, unsigned& e) {
    T = s.cut ? s.prefix : 0xffffffffu;
    e = s.cut ? s.krem : 0x7fffffffu;
}

__global__ __launch_bounds__(SMP_THREADS) void sample_count(SmpArgs a) {
    __shared__ int red[SMP_WAVES];
    __shared__ unsigned dl[4];
    const int b = blockIdx.y;
    SelState st[2];
    ImgInfo info;
    resolve_level(a, b, 3, st, &info, red, dl);
    unsigned Tf, ef, Tb, eb;
    cut_of(st[0], Tf, ef);
    cut_of(st[1], Tb, eb);
    const bool skipped = image_skipped(a, b);
    int lt_f = 0, eq_f = 0, eq_b = 0;
    Item items[SMP_TILES];
    load_span(a, b, skipped, st[0].cut, st[1].cut, false, items);
#pragma unroll
    for (int tile = 0; tile < SMP_TILES; ++tile) {
        const Item it = items[tile];
        lt_f += it.kind == KIND_FG && (!st[0].cut || it.key < Tf);           // a class that is not cut is taken whole
        eq_f += it.kind == KIND_FG && st[0].cut && it.key == Tf;
        eq_b += it.kind == KIND_BG && st[1].cut && it.key == Tb;
    }
    const int s0 = block_sum(lt_f, red), s1 = block_sum(eq_f, red), s2 = block_sum(eq_b, red);
    if (threadIdx.x == 0) {
        int* o = a.cnt1 + ((long long)b * a.nwg + blockIdx.x) * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = 0;
    }
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(SMP_THREADS) void sample_mark(SmpArgs a) {
    __shared__ int red[SMP_WAVES];
    const int b = blockIdx.y, me = blockIdx.x;
    const SelState* stp = a.state + ((long long)3 * a.B + b) * 2;
    const SelState sf = stp[0], sb = stp[1];
    unsigned Tf, ef, Tb, eb;
    cut_of(sf, Tf, ef);
    cut_of(sb, Tb, eb);
    // what the workgroups in front of this one hold: foreground at T, background at T, sampled foreground
    long long carry = 0;                                      // foreground at T in the chunks already passed
    int acc_eqf = 0, acc_eqb = 0, acc_sel = 0;
    for (int chunk = 0; chunk <= me; chunk += SMP_THREADS) {  // uniform
        const int w = chunk + threadIdx.x;
        int lt = 0, qf = 0, qb = 0;
        if (w < a.nwg) {
            const int* c = a.cnt1 + ((long long)b * a.nwg + w) * 4;
            lt = c[0]; qf = c[1]; qb = c[2];
        }
        unsigned total;
        const long long before = carry + block_excl_scan((unsigned)qf, red, total);
        carry += total;
        if (w < me) {
            acc_eqf += qf;
            acc_eqb += qb;
            acc_sel += lt + (int)clampll((long long)ef - before, 0, qf);
        }
    }
    long long base_eqf = block_sum(acc_eqf, red);
    long long base_eqb = block_sum(acc_eqb, red);
    long long base_sel = block_sum(acc_sel, red);
    const int total_fg = (int)sf.take;
    const bool skipped = image_skipped(a, b);

    Item items[SMP_TILES];
    load_span(a, b, skipped, true, true, true, items);
#pragma unroll
    for (int tile = 0; tile < SMP_TILES; ++tile) {
        const int r0 = me * SMP_SPAN + tile * SMP_THREADS;
        if (r0 >= a.R) break;                                 // uniform
        const int r = r0 + threadIdx.x;
        const bool live = r < a.R;
        const Item it = items[tile];
        const bool qf = it.kind == KIND_FG && sf.cut && it.key == Tf;
        const bool qb = it.kind == KIND_BG && sb.cut && it.key == Tb;
        unsigned tot;
        const unsigned ex = block_excl_scan((unsigned)qf | ((unsigned)qb << 16), red, tot);   // at most 256 of each per tile
        bool sel = false;
        if (it.kind == KIND_FG) sel = !sf.cut || it.key < Tf || (qf && base_eqf + (long long)(ex & 0xffffu) < (long long)ef);
        if (it.kind == KIND_BG) sel = !sb.cut || it.key < Tb || (qb && base_eqb + (long long)(ex >> 16) < (long long)eb);
        base_eqf += tot & 0xffffu;
        base_eqb += tot >> 16;
        const bool self = sel && it.kind == KIND_FG;
        unsigned tots;
        const unsigned pos = block_excl_scan((unsigned)self, red, tots);
        if (live) {
            const long long row = (long long)b * a.R + r;
            a.labels[row] = it.kind == KIND_FG ? it.label : (it.kind == KIND_IGN ? SMP_IGN : 0);          // :470-472
            a.bbox_weights[row] = self ? 1.0f : 0.0f;                                                      // :612
            a.labels_scores[row] = it.kind == KIND_IGN ? 0.0f : it.score;                                  // :886-887
            a.sampled[row] = sel ? (unsigned char)it.kind : (unsigned char)0;                              // :610-611
            const long long p = base_sel + pos;
            if (self && p < a.R) a.fg_index[(long long)b * a.R + p] = r;
            if (r >= total_fg) a.fg_index[row] = -1;
        }
        base_sel += tots;
    }
    if (me == 0 && threadIdx.x == 0) {
        const ImgInfo in = a.info[b];
        int32_t* c = a.counts + (long long)b * 6;
        c[0] = in.n_fg; c[1] = in.n_bg; c[2] = in.fg_num; c[3] = in.bg_num; c[4] = (int)sf.take; c[5] = (int)sb.take;
        a.fg_counts[b] = total_fg;
    }
}

int smp_nwg(int R) { return (R + SMP_SPAN - 1) / SMP_SPAN; }

struct SmpLayout { size_t hist, cnt0, cnt1, state, info, total; };
SmpLayout smp_layout(int B, int R) {
    SmpLayout L;
    const size_t n = (size_t)B * smp_nwg(R);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = gnms_align_up(o + bytes, 16); return r; };
    L.hist = take(2 * n * 512 * sizeof(unsigned));
    L.cnt0 = take(n * 2 * sizeof(int));
    L.cnt1 = take(n * 4 * sizeof(int));
    L.state = take((size_t)4 * B * 2 * sizeof(SelState));
    L.info = take((size_t)B * sizeof(ImgInfo));
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------ classification term

struct ClsArgs {
    const float* cls;            // [B][R][C]
    const long long* labels;
    const float* labels_scores;
    const unsigned char* sampled;
    const int32_t* counts;       // [B][6]
    int B, R, C, nwg;
    int has_ff;
    double ff, focal;
    float lambda;
    float* labels_weight;
    float* loss;
    float* dcls;
    double* acc;
    int32_t* stat_counts;        // fg correct, fg all, bg correct, bg all, active
    double* wsum;                // [B * nwg]
    int* wact;                   // [B * nwg]     active anchors (dense: every workgroup of cls_loss_finish sums all of them)
    int* wint;                   // [B * nwg][4]  fg correct, fg all, bg correct, bg all
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int s = 1; s < GNMS_WAVE; s <<= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ __forceinline__ double block_sum_f64(double v, double* redd) {
    const int lane = threadIdx.x & (GNMS_WAVE - 1), wave = threadIdx.x / GNMS_WAVE;
    v = wave_sum_f64(v);
    __syncthreads();
    if (lane == 0) redd[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) t += redd[w];
    return t;
}

__global__ __launch_bounds__(SMP_THREADS) void cls_loss_main(ClsArgs a) {
    __shared__ int red[SMP_WAVES];
    __shared__ double redd[SMP_WAVES];
    const int b = blockIdx.y;
    // :913-938: the batch's sampled totals and the foreground weight, float64
    int f = 0, g = 0;
    for (int i = threadIdx.x; i < a.B; i += SMP_THREADS) { f += a.counts[(long long)i * 6 + 4]; g += a.counts[(long long)i * 6 + 5]; }
    const int fg_tot = block_sum(f, red), bg_tot = block_sum(g, red);
    double fgw = 1.0;
    if (a.has_ff && fg_tot > 0) fgw = (a.ff / (1.0 - a.ff)) * ((double)bg_tot / (double)fg_tot);

    double sum = 0.0;
    int n_act = 0, fg_ok = 0, fg_all = 0, bg_ok = 0, bg_all = 0;
    for (int tile = 0; tile < CLS_TILES; ++tile) {
        const int r = blockIdx.x * CLS_SPAN + tile * SMP_THREADS + threadIdx.x;
        if (r >= a.R) break;
        const long long row = (long long)b * a.R + r;
        const int s = a.sampled[row];
        const long long label = a.labels[row];
        double w64 = s == KIND_FG ? fgw : 1.0;
        if (a.focal != 0.0) {                                                  // :945-961
            const double u = 1.0 - (double)a.labels_scores[row];
            w64 *= a.focal == 2.0 ? u * u : pow(u, a.focal);                   // (NumPy squares for an exponent of 2)
        }
        const float w = (s == KIND_FG || s == KIND_BG) ? (float)w64 : 0.0f;    // :971
        a.labels_weight[row] = w;
        const float* x = a.cls + row * a.C;
        float* d = a.dcls + row * a.C;
        // argmax (the first maximum; a NaN is the maximum) and the row maximum
        float m = x[0];
        int arg = 0;
        for (int c = 1; c < a.C; ++c) {
            const float v = x[c];
            if (m == m && (v != v || v > m)) { m = v; arg = c; }
        }
        if (label > 0 && label != SMP_IGN) { ++fg_all; fg_ok += arg == label; }     // :893-907
        else if (label == 0) { ++bg_all; bg_ok += arg == 0; }
        const bool active = w > 0.0f && label >= 0 && label < a.C;                  // :979
        bool grad = false;
        float lse = 0.0f;
        if (active) {
            float se = 0.0f;
            for (int c = 0; c < a.C; ++c) se += expf(x[c] - m);
            lse = logf(se);
            const float ce = -((x[label] - m) - lse);
            const float wl = ce * w;                                                // :990
            grad = wl >= 0.0f && wl <= 2000.0f;
            const float v = wl < 0.0f ? 0.0f : (wl > 2000.0f ? 2000.0f : wl);       // :993 (a NaN stays)
            sum += (double)v;
            ++n_act;
        }
        for (int c = 0; c < a.C; ++c) d[c] = grad ? w * (expf((x[c] - m) - lse) - (c == label ? 1.0f : 0.0f)) : 0.0f;
    }
    const double ssum = block_sum_f64(sum, redd);
    const int i0 = block_sum(n_act, red), i1 = block_sum(fg_ok, red), i2 = block_sum(fg_all, red), i3 = block_sum(bg_ok, red),
              i4 = block_sum(bg_all, red);
    if (threadIdx.x == 0) {
        const long long slot = (long long)b * a.nwg + blockIdx.x;
        a.wsum[slot] = ssum;
        a.wact[slot] = i0;
        int* o = a.wint + slot * 4;
        o[0] = i1; o[1] = i2; o[2] = i3; o[3] = i4;
    }
}

__global__ __launch_bounds__(SMP_THREADS) void cls_loss_finish(ClsArgs a) {
    __shared__ int red[SMP_WAVES];
    __shared__ double redd[SMP_WAVES];
    const int nslots = a.B * a.nwg;
    int n = 0;
    for (int i = threadIdx.x; i < nslots; i += SMP_THREADS) n += a.wact[i];
    const int n_act = block_sum(n, red);
    if (blockIdx.x == 0) {
        double s = 0.0;
        int v[4] = {0, 0, 0, 0};
        for (int i = threadIdx.x; i < nslots; i += SMP_THREADS) {
            s += a.wsum[i];
            for (int k = 0; k < 4; ++k) v[k] += a.wint[(long long)i * 4 + k];
        }
        s = block_sum_f64(s, redd);
        for (int k = 0; k < 4; ++k) v[k] = block_sum(v[k], red);
        if (threadIdx.x == 0) {
            // :996-997: the mean (float64 sum, one rounding), then times lambda in float32
            a.loss[0] = (n_act > 0 && a.lambda != 0.0f) ? (float)(s / (double)n_act) * a.lambda : 0.0f;
            a.acc[0] = (double)v[0] / (double)v[1];           // 0 / 0 = NaN: no foreground label in the batch
            a.acc[1] = (double)v[2] / (double)v[3];
            a.stat_counts[0] = v[0]; a.stat_counts[1] = v[1]; a.stat_counts[2] = v[2]; a.stat_counts[3] = v[3];
            a.stat_counts[4] = n_act;
        }
    }
    const float scale = (n_act > 0 && a.lambda != 0.0f) ? a.lambda / (float)n_act : 0.0f;
    const long long total = (long long)a.B * a.R * a.C;
    const long long i0 = (long long)blockIdx.x * (SMP_THREADS * FIN_ELEMS) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < FIN_ELEMS; ++k) {
        const long long i = i0 + (long long)k * SMP_THREADS;
        if (i < total) a.dcls[i] = scale != 0.0f ? a.dcls[i] * scale : 0.0f;
    }
}

int cls_nwg(int R) { return (R + CLS_SPAN - 1) / CLS_SPAN; }

}  // namespace

extern "C" size_t gnms_sample_anchors_workspace_bytes(int B, int R) {
    if (B <= 0 || R <= 0) return 0;
    return smp_layout(B, R).total;
}

extern "C" int gnms_sample_anchors(const float* target_labels, int64_t ld_target_labels, const float* prob, const uint8_t* skip, int B, int R,
                                   int C, double box_samples, int has_fg_fraction, double fg_fraction, int64_t* labels,
                                   float* bbox_weights, float* labels_scores, uint8_t* sampled, int32_t* fg_index, int32_t* fg_counts,
                                   int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 0, "gnms_sample_anchors: B = %d", B);
    GNMS_CHECK_ARG(R >= 1, "gnms_sample_anchors: R = %d < 1", R);
    GNMS_CHECK_ARG(C >= 2, "gnms_sample_anchors: C = %d < 2 (background and at least one class)", C);
    GNMS_CHECK_ARG(B <= 65535, "gnms_sample_anchors: B = %d > 65535", B);
    GNMS_CHECK_ARG(R < (1 << 30) && (long long)R * C < (1ll << 40), "gnms_sample_anchors: R = %d too large", R);
    GNMS_CHECK_ARG(box_samples >= 0.0, "gnms_sample_anchors: box_samples = %g", box_samples);
    GNMS_CHECK_ARG(isinf(box_samples) || (has_fg_fraction && fg_fraction == fg_fraction),
                   "gnms_sample_anchors: a finite box_samples needs fg_fraction");
    GNMS_CHECK_ARG(labels && bbox_weights && labels_scores && sampled && fg_index && fg_counts && counts,
                   "gnms_sample_anchors: an output is NULL");
    if (B == 0) return GNMS_OK;
    GNMS_CHECK_ARG(target_labels && prob, "gnms_sample_anchors: target_labels / prob is NULL");
    GNMS_CHECK_ARG(ld_target_labels >= 1, "gnms_sample_anchors: ld_target_labels = %lld", (long long)ld_target_labels);
    const SmpLayout L = smp_layout(B, R);
    if (!workspace || workspace_bytes < L.total) {
        gnms_set_error("gnms_sample_anchors: workspace of %zu bytes, needs %zu", workspace_bytes, L.total);
        return GNMS_ERR_WORKSPACE;
    }
    GNMS_CHECK_ARG((uintptr_t)workspace % 16 == 0, "gnms_sample_anchors: workspace must be 16-byte aligned");

    SmpArgs a = {};
    a.tl = target_labels; a.ld_tl = ld_target_labels; a.prob = prob; a.skip = skip;
    a.B = B; a.R = R; a.C = C; a.nwg = smp_nwg(R);
    a.box_samples = box_samples; a.fg_fraction = has_fg_fraction ? fg_fraction : 0.0;
    a.labels = (long long*)labels; a.bbox_weights = bbox_weights; a.labels_scores = labels_scores; a.sampled = sampled;
    a.fg_index = fg_index; a.fg_counts = fg_counts; a.counts = counts;
    char* ws = static_cast<char*>(workspace);
    a.hist = reinterpret_cast<unsigned*>(ws + L.hist);
    a.cnt0 = reinterpret_cast<int*>(ws + L.cnt0);
    a.cnt1 = reinterpret_cast<int*>(ws + L.cnt1);
    a.state = reinterpret_cast<SelState*>(ws + L.state);
    a.info = reinterpret_cast<ImgInfo*>(ws + L.info);

    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(a.nwg, B);
    sample_hist<0><<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    sample_hist<1><<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    sample_hist<2><<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    sample_hist<3><<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    sample_count<<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    sample_mark<<<grid, SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" size_t gnms_cls_loss_workspace_bytes(int B, int R) {
    if (B <= 0 || R <= 0) return 0;
    return (size_t)B * cls_nwg(R) * (sizeof(double) + 5 * sizeof(int));
}

extern "C" int gnms_cls_loss(const float* cls, const int64_t* labels, const float* labels_scores, const uint8_t* sampled,
                             const int32_t* counts, int B, int R, int C, int has_fg_fraction, double fg_fraction, double focal_loss,
                             double cls_2d_lambda, float* labels_weight, float* loss, float* dcls, double* acc, int32_t* stat_counts,
                             void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 1, "gnms_cls_loss: B = %d < 1", B);
    GNMS_CHECK_ARG(R >= 1, "gnms_cls_loss: R = %d < 1", R);
    GNMS_CHECK_ARG(C >= 2, "gnms_cls_loss: C = %d < 2 (background and at least one class)", C);
    GNMS_CHECK_ARG(B <= 65535, "gnms_cls_loss: B = %d > 65535", B);
    GNMS_CHECK_ARG(R < (1 << 30) && (long long)B * R * C < (1ll << 40) && (long long)B * cls_nwg(R) < (1ll << 31),
                   "gnms_cls_loss: B = %d, R = %d too large", B, R);
    GNMS_CHECK_ARG(!has_fg_fraction || fg_fraction == fg_fraction, "gnms_cls_loss: fg_fraction is NaN");
    GNMS_CHECK_ARG(focal_loss == focal_loss && cls_2d_lambda == cls_2d_lambda, "gnms_cls_loss: focal_loss / cls_2d_lambda is NaN");
    GNMS_CHECK_ARG(labels_weight && loss && dcls && acc && stat_counts, "gnms_cls_loss: an output is NULL");
    GNMS_CHECK_ARG(cls && labels && labels_scores && sampled && counts, "gnms_cls_loss: an input is NULL");
    const size_t need = gnms_cls_loss_workspace_bytes(B, R);
    if (!workspace || workspace_bytes < need) {
        gnms_set_error("gnms_cls_loss: workspace of %zu bytes, needs %zu", workspace_bytes, need);
        return GNMS_ERR_WORKSPACE;
    }
    GNMS_CHECK_ARG((uintptr_t)workspace % 8 == 0, "gnms_cls_loss: workspace must be 8-byte aligned");

    ClsArgs a = {};
    a.cls = cls; a.labels = (const long long*)labels; a.labels_scores = labels_scores; a.sampled = sampled; a.counts = counts;
    a.B = B; a.R = R; a.C = C; a.nwg = cls_nwg(R);
    a.has_ff = has_fg_fraction != 0; a.ff = fg_fraction; a.focal = focal_loss; a.lambda = (float)cls_2d_lambda;
    a.labels_weight = labels_weight; a.loss = loss; a.dcls = dcls; a.acc = acc; a.stat_counts = stat_counts;
    a.wsum = static_cast<double*>(workspace);
    a.wact = reinterpret_cast<int*>(a.wsum + (size_t)B * a.nwg);
    a.wint = a.wact + (size_t)B * a.nwg;

    hipStream_t st = (hipStream_t)stream;
    cls_loss_main<<<dim3(a.nwg, B), SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    const long long total = (long long)B * R * C;
    const long long per = (long long)SMP_THREADS * FIN_ELEMS;
    cls_loss_finish<<<(unsigned)((total + per - 1) / per), SMP_THREADS, 0, st>>>(a);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
