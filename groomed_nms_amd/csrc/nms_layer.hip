// nms_layer.hip -- host side of the GrooMeD-NMS C ABI: argument checks, workspace carving, launches.
// Kernels: nms_kernels.h / nms_layer_kernels.h (forward), nms_backward_kernels.h, nms_solve_kernels.h, nms_one_launch.h.
// Not here: tail_kernel and tail_write_kernel with their launchers (the nms_tail_*.hip / nms_tail_write_*.hip units) and the
// gnms_profile_* entries (nms_profile.hip); nms_layer.h is what these units share, and its definitions are in this file.
#include <stdarg.h>
#include <string.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <atomic>
#include <vector>
#include "gnms_prof.h"
#include "iou_tile.h"
#include "iou3d_tile.h"
#include "iou3d_sym.h"
#include "nms_layer_kernels.h"
#include "nms_solve_kernels.h"
#include "nms_one_launch.h"
#include "nms_writers.h"
#include "nms_layer.h"

// defined in iou_kernels.hip
bool gnms_internal_overlap3d_sym_ok(int N, int64_t ld, const float* out);
int gnms_internal_nms_overlap3d_sym(const float* rec, int B, int N, float* out, int64_t ld, hipStream_t st, float thr, int pct0, int pct1,
                                    int leave_cus = 0, int force_persist = 0);
int gnms_internal_iou2d_rows(const float* boxes, int B, int N, float* out, int64_t ld, hipStream_t st, int row0, int row_end);

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void gnms_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* gnms_last_error(void) { return g_err; }

// compute units of the current device, cached per device (declared in gnms_common.h)
int gnms_device_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> lock(mu);
    int& c = cus[dev];
    if (c == 0) {
        hipDeviceProp_t prop;
        c = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return c;
}
extern "C" int gnms_abi_version(void) { return GNMS_ABI_VERSION; }

extern "C" void gnms_default_params(gnms_params* p) {
    if (!p) return;
    p->nms_threshold = 0.4f;             // lib/groomed_nms.py:10 defaults
    p->temperature = 0.01f;
    p->valid_box_prob_threshold = 0.3f;
    p->pruning_method = GNMS_PRUNE_LINEAR;
    p->return_sorted_prob = 0;
    p->group_boxes = 1;
    p->mask_group_boxes = 1;
    p->group_size = 100;
    p->presorted = 0;
}

// Kernels that need more than 64 KiB of dynamic LDS must be told so once per (device, kernel); the attribute call is not free
// (a driver round trip per launch adds up on the small-N path), so what has been granted is remembered.  (Declared in gnms_common.h.)
int gnms_allow_lds_raw(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return GNMS_OK;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> granted;
    int dev = 0;
    GNMS_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t& g = granted[std::make_pair(dev, kernel)];
    if (g >= bytes) return GNMS_OK;
    GNMS_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    g = bytes;
    return GNMS_OK;
}

// ------------------------------------------------------------------------------------------------
// what the layer's units share (nms_layer.h): the one definition of each
// ------------------------------------------------------------------------------------------------
namespace gnms {

int next_pow2(int n) {
    int p = 64;               // block_sort works on >= 64 keys (one wave)
    while (p < n) p <<= 1;
    return p;
}

size_t leaders_lds_bytes(int N) { return leaders_lds_size((N + 63) / 64); }

int check_common(const char* fn, int B, int N, int64_t ld, const gnms_params* P, const void* ws, size_t ws_bytes) {
    GNMS_CHECK_ARG(P != nullptr, "%s: params is NULL", fn);
    GNMS_CHECK_ARG(B >= 0 && N >= 0, "%s: negative size (B=%d N=%d)", fn, B, N);
    GNMS_CHECK_ARG(ld >= N, "%s: ld (%lld) < N (%d)", fn, (long long)ld, N);
    if (N > GNMS_MAX_BOXES) {
        gnms_set_error("%s: N=%d exceeds GNMS_MAX_BOXES=%d", fn, N, GNMS_MAX_BOXES);
        return GNMS_ERR_UNSUPPORTED;
    }
    if (P->pruning_method < 0 || P->pruning_method > 2) {
        gnms_set_error("%s: Pruning method not implemented! (pruning_method=%d)", fn, P->pruning_method);   // lib/groomed_nms.py:178
        return GNMS_ERR_UNSUPPORTED;
    }
    GNMS_CHECK_ARG(P->group_size >= 0, "%s: group_size < 0", fn);
    if (P->group_boxes && !P->mask_group_boxes && (long long)P->group_size + 1 > kGroupMaxMembers && N > kGroupMaxMembers) {
        gnms_set_error("%s: unmasked groups support group_size+1 <= %d", fn, kGroupMaxMembers);
        return GNMS_ERR_UNSUPPORTED;
    }
    if (B > 0 && N > 0) {
        GNMS_CHECK_ARG(ws != nullptr, "%s: workspace is NULL", fn);
        if (ws_bytes < gnms_workspace_bytes(B, N, P)) {
            gnms_set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, gnms_workspace_bytes(B, N, P));
            return GNMS_ERR_WORKSPACE;
        }
        GNMS_CHECK_ARG((uintptr_t)ws % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
    }
    return GNMS_OK;
}

// K2, the one full read of the matrix: workgroups of 8 waves (2048 columns side by side), 16 from N = 4096 (whole 16-KiB rows), eight
// one-KiB loads in flight per wave.
// The matrix-in layer decides on the device whether the thresholded matrix is symmetric (every caller in the reference passes
// iou(boxes, boxes)): bitmask_kernel then stores the rows of W in full and wsym_check_kernel compares the 64 x 64 blocks with
// their transposes; K3 / K4 (sym = 2) take the pulling, attributing scan for the images that pass.  GNMS_MATRIX_SYM=0: never.
// The row-buffer kernels' rows of W leave as 16-byte write-through stores (w_rows_write_through, nms_kernels.h) on the routes in this mask.
// GNMS_W_WRITE_THROUGH=0: plain stores everywhere (developer / test switch, read once: both forms stay reachable in one build for A/B runs
// and the tests); another number is taken as the mask itself (kWtKbw2 = 1, kWtKbw1 = 2, kWtChunkLoop = 4, kWtMatrixIn = 8), for A/B runs
// of a single route.
// Measured per route (LABNOTES R9, ms per step, three alternating runs, parent / change): two blocks per workgroup (B = 8, N = 4096) 0.1317-0.1318 /
// 0.1290-0.1291; one block (B = 4) 0.0833-0.0836 / 0.0809-0.0818; matrix-in (--two-calls) 0.2362-0.2379 / 0.2352-0.2361.  The chunk loop
// (B = 32, N = 4096: W is 67 MB, twice the L2, and streams through it anyway) shows no difference between the two forms and keeps the plain store.
constexpr int kWtDefaultRoutes = kWtKbw2 | kWtKbw1 | kWtMatrixIn;
// A developer / test switch: the number in the environment variable `name`, `dflt` where it is unset or empty.  Every switch reads its
// variable once, into a function-local static, so both forms of what it selects stay reachable in one build for A/B runs and the tests.
int env_switch(const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; }
int w_write_through_routes() { static const int routes = env_switch("GNMS_W_WRITE_THROUGH", kWtDefaultRoutes); return routes; }
bool matrix_sym_detection(int N) {
    static const int forced = env_switch("GNMS_MATRIX_SYM", -1);
    return forced >= 0 ? forced != 0 : N >= 256;
}

LayerCall make_call(int B, int N, const int32_t* counts, const gnms_params& P, void* workspace, void* stream, float* prob, int64_t* order,
                    int64_t* valid, int64_t* invalid, int32_t* nvalid, int32_t* ninvalid) {
    return LayerCall{B, N, counts, P, gnms_make_layout(N), (char*)workspace, (hipStream_t)stream, next_pow2(N), prob, order, valid, invalid, nvalid, ninvalid};
}
// the prologue of an entry (nms_layer.h)
int begin_call(const char* fn, LayerCall* c, int B, int N, int64_t ld, const int32_t* counts, const gnms_params* params, void* workspace,
               size_t workspace_bytes, void* stream, bool without_matrix, bool ptrs_ok, const char* null_msg, float* prob, int64_t* order,
               int64_t* valid, int64_t* invalid, int32_t* nvalid, int32_t* ninvalid) {
    int rc = check_common(fn, B, N, ld, params, workspace, workspace_bytes);
    if (rc) return rc;
    if (without_matrix && (!params->group_boxes || params->presorted)) {
        gnms_set_error("%s: only the grouped, hard-sorted modes run without the matrix", fn);
        return GNMS_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return kCallEmpty;
    if (N == 0) {
        if (nvalid) GNMS_CHECK_HIP(hipMemsetAsync(nvalid, 0, sizeof(int32_t) * B, st));
        if (ninvalid) GNMS_CHECK_HIP(hipMemsetAsync(ninvalid, 0, sizeof(int32_t) * B, st));
        return kCallEmpty;
    }
    GNMS_CHECK_ARG(ptrs_ok, "%s", null_msg);
    *c = make_call(B, N, counts, *params, workspace, stream, prob, order, valid, invalid, nvalid, ninvalid);
    return GNMS_OK;
}

// K3..K6 in one launch (masked groups): the fast tail (nms_kernels.h) is on unless GNMS_FAST_TAIL=0 (developer switch: the K5-proper path
// stays reachable for A/B runs and tests)
bool fast_tail_enabled() { static const bool on = env_switch("GNMS_FAST_TAIL", 1) != 0; return on; }

// dynamic LDS of the chain in tail_kernel / tail_write_kernel; P2: the launch's key count (>= 1024: the fused kernels always run 1024 threads)
size_t tail_lds_bytes(int N, int P2, int fast) {
    // (the fused K5 -> K6 hand-off, E <= 4, parks order[] and a copy of r2 behind the key region: 16 bytes per key)
    const size_t llds = leaders_lds_bytes(N), glds = (size_t)P2 * (P2 <= 4096 ? 16 : 8);
    size_t lds = llds > glds ? llds : glds;
    if (fast && lds < fast_tail_lds_size(N, P2)) lds = fast_tail_lds_size(N, P2);
    return lds;
}

}  // namespace gnms

using namespace gnms;

namespace {
// The gates of the forward and backward entries, each written ONCE: the entries below branch on them and gnms_backward_reads answers
// from them, so what a binding keeps for the backward cannot drift from what the library runs.
bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }                 // the from-boxes kernels load a box as one float4
bool masked_groups(const gnms_params& P) { return P.group_boxes && P.mask_group_boxes; }   // their backward reads no overlap
// gnms_forward_with_iou2d runs the layer from the boxes (gnms_backward_from_boxes can follow when the groups are unmasked)
bool from_boxes_2d(const gnms_params& P, const void* boxes) { return P.group_boxes && !P.presorted && aligned16(boxes); }
// gnms_forward_with_iou3d runs the layer from the cuboid records
bool from_records_3d(const gnms_params& P) { return masked_groups(P) && !P.presorted; }
// masked groups, hard sort, unsorted output (the default mode): gnms_backward fuses its first pass into the masked kernel, and
// gnms_backward_boxes has one matrix-gradient entry per non-head member -- no N x N pass
bool masked_default(const gnms_params& P) { return masked_groups(P) && !P.return_sorted_prob && !P.presorted; }
bool boxes_sparse_route(const gnms_params& P, int route) { return route == GNMS_BOXES_ROUTE_AUTO && masked_default(P); }
}  // namespace

// host code only (the gate table stands in include/groomed_nms_hip.h)
extern "C" int gnms_backward_reads(int entry, const gnms_params* params, const void* boxes, int box_grad_route) {
    GNMS_CHECK_ARG(entry >= GNMS_ENTRY_MATRIX && entry <= GNMS_ENTRY_FROM_BOXES, "gnms_backward_reads: unknown entry %d", entry);
    GNMS_CHECK_ARG(params != nullptr, "gnms_backward_reads: params is NULL");
    GNMS_CHECK_ARG(boxes != nullptr || entry == GNMS_ENTRY_MATRIX, "gnms_backward_reads: boxes is NULL");
    const gnms_params& P = *params;
    if (box_grad_route != GNMS_BOXES_ROUTE_NONE) {
        GNMS_CHECK_ARG(box_grad_route == GNMS_BOXES_ROUTE_AUTO || box_grad_route == GNMS_BOXES_ROUTE_DENSE, "gnms_backward_reads: unknown route %d",
                       box_grad_route);
        GNMS_CHECK_ARG(entry == GNMS_ENTRY_WITH_IOU2D || entry == GNMS_ENTRY_FROM_BOXES,
                       "gnms_backward_reads: gnms_backward_boxes follows gnms_forward_with_iou2d / gnms_forward_from_boxes only");
        return GNMS_BWD_READS_BOXES | (boxes_sparse_route(P, box_grad_route) ? 0 : GNMS_BWD_READS_MATRIX) | (aligned16(boxes) ? 0 : GNMS_BWD_COPY_BOXES);
    }
    if (entry == GNMS_ENTRY_MATRIX) return GNMS_BWD_READS_MATRIX;
    if (entry == GNMS_ENTRY_FROM_BOXES) return GNMS_BWD_READS_BOXES | GNMS_BWD_FROM_BOXES;
    if (masked_groups(P)) return 0;
    if (entry == GNMS_ENTRY_WITH_IOU2D && from_boxes_2d(P, boxes)) return GNMS_BWD_READS_BOXES | GNMS_BWD_FROM_BOXES;
    return GNMS_BWD_READS_MATRIX;
}

// full: 0 = only the words a leader scan reads; 1 = whole rows + wsym_check_kernel behind; 2 = whole rows, the check rides in the tail launch
int gnms_internal_launch_bitmask(const LayerCall& c, const float* iou, int64_t ld, int full) {
    const int B = c.B, N = c.N;
    const gnms_ws_layout& L = c.L;
    // (measured at B = 8, N = 4096, three interleaved repetitions: 16 waves 91.6-91.8 us = 0.733 of the HBM peak, 8 waves 95.2-95.7 us;
    // 16 loads in flight per wave change nothing either way)
    const bool vec = (ld % 4 == 0) && ((uintptr_t)iou % 16 == 0);
    const int wt = w_write_through_routes() & kWtMatrixIn;           // (only the 16-wave kernel has the row buffer)
#define GNMS_BITMASK(V, W, R)                                                                                                         \
    gnms_launch_prof(kProfMatrixRead, bitmask_kernel<V, W, R>, dim3(gnms_div_up(N, W * 256), L.NB, B), dim3(W * 64), 0, c.st, iou, N, (long)ld, c.counts, c.P.nms_threshold, c.ws, L, full, wt)
    // few, small images: one batch of loads per wave instead of eight in a row (bitmask_small_kernel)
    constexpr int small_wgs = 1024;
    if (!vec) GNMS_BITMASK(false, kMaskWaves, kMaskRB);
    else if (N <= 2048 && (long)B * L.NB * gnms_div_up(N, 256) <= (long)small_wgs)        // (N = 4096, B = 1 keeps the row-buffered 16-wave kernel)
        gnms_launch_prof(kProfMatrixRead, bitmask_small_kernel, dim3(gnms_div_up(N, 256), L.NB, B), dim3(512), 0, c.st, iou, N, (long)ld, c.counts, c.P.nms_threshold, c.ws, L, full);
    else if (N >= 4096) GNMS_BITMASK(true, 16, 8);
    else GNMS_BITMASK(true, 8, 8);
#undef GNMS_BITMASK
    GNMS_CHECK_LAUNCH();
    if (full == 1) {
        const int nb = (N + 63) / 64;
        wsym_check_kernel<<<dim3(gnms_div_up(nb * (nb + 1) / 2, 4), B), 256, 0, c.st>>>(N, c.counts, c.ws, L);
        GNMS_CHECK_LAUNCH();
    }
    return GNMS_OK;
}

namespace {

// the direction of the per-group solves (solve_groups_kernel's BWD)
constexpr bool kForward = false, kBackward = true;

// ------------------------------------------------------------------------------------------------
// K3..K6 as launches of their own, one launcher per block; src / ld: the overlaps' source (SRC: kFromMatrix, kFromBoxes, kFromRecords)
// ------------------------------------------------------------------------------------------------
// K3 + K4: the leader scan and the attribution, behind the bit matrix
template <int SRC>
int launch_leaders_attribute(const LayerCall& c, const float* src, int64_t ld, int sym) {
    const size_t lds = leaders_lds_bytes(c.N);
    int rc = allow_lds(leaders_kernel, lds);
    if (rc) return rc;
    const int spw = leaders_chain_wgs(c.N, sym);
    leaders_kernel<<<c.B * spw, 1024, lds, c.st>>>(c.N, c.counts, c.ws, c.L, sym, c.B, spw);
    GNMS_CHECK_LAUNCH();
    attribute_kernel<SRC><<<dim3(c.L.NB, c.B), 64, 0, c.st>>>(src, (long)ld, c.N, c.counts, c.P.nms_threshold, c.ws, c.L, sym);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
// K5
template <int SRC>
int launch_groups(const LayerCall& c, const float* src, int64_t ld) {
    int rc;
    GNMS_DISPATCH_SORT(c.P2, {
        if ((rc = allow_lds(groups_kernel<E, SRC>, c.sort_lds()))) return rc;
        groups_kernel<E, SRC><<<c.B, c.sort_threads(), c.sort_lds(), c.st>>>(src, c.N, (long)ld, c.counts, c.P, c.ws, c.L, c.P2);
    });
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
// unmasked groups: the per-group solves, forward (between K5 and K6) and backward
template <bool BWD, int SRC>
int launch_solve_groups(const LayerCall& c, const float* src, int64_t ld, float* grad_scores, float* grad_src) {
    int rc;
    if ((rc = allow_lds(solve_groups_kernel<BWD, SRC == kFromBoxes>, kSolveGroupsLds))) return rc;
    solve_groups_kernel<BWD, SRC == kFromBoxes><<<dim3(solve_groups_wgs(c.B, gnms_device_cu_count()), c.B), 1024, kSolveGroupsLds, c.st>>>(
        src, c.N, (long)ld, c.counts, c.P, c.ws, c.L, grad_scores, grad_src);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
// K6
int launch_finalize(const LayerCall& c) {
    int rc;
    GNMS_DISPATCH_SORT(c.P2, {
        if ((rc = allow_lds(finalize_kernel<E>, c.sort_lds()))) return rc;
        finalize_kernel<E><<<c.B, c.sort_threads(), c.sort_lds(), c.st>>>(c.N, c.counts, c.P, c.ws, c.L, c.P2, c.prob, (long long*)c.valid, (long long*)c.invalid,
                                                                            c.nvalid, c.ninvalid);
    });
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
// K3..K6 behind the bit matrix, where they do not run as one launch (launch_tail, launch_tail_write)
template <int SRC>
int launch_separate_tail(const LayerCall& c, const float* src, int64_t ld, int sym) {
    int rc;
    if ((rc = launch_leaders_attribute<SRC>(c, src, ld, sym))) return rc;
    if ((rc = launch_groups<SRC>(c, src, ld))) return rc;
    if constexpr (SRC != kFromRecords) {                          // (the from-records layer runs masked groups only)
        if (!c.P.mask_group_boxes && (rc = launch_solve_groups<kForward, SRC>(c, src, ld, nullptr, nullptr))) return rc;
    }
    return launch_finalize(c);
}

}  // namespace

extern "C" size_t gnms_workspace_bytes(int B, int N, const gnms_params* params) {
    if (B <= 0 || N <= 0) return 0;
    size_t bytes = gnms_make_layout(N).per_image * (size_t)B;
    if (params && !params->group_boxes) bytes += gnms::ungrouped_scratch_bytes(B, N);   // the sorted strictly-lower-triangular matrix
    return bytes;
}

namespace {

// gnms_iou2d of a box set WITH ITSELF (what both reference call sites compute: iou(boxes, boxes)), N <= 4096: the staged writers as a
// launch of their own -- the same claimed units, tile body and cached columns as in tail_write_kernel, the claim counters in a zeroed
// array that lives for the call.  (A version that dealt the units statically -- round robin per image, no counters -- reached 0.55 of
// the HBM peak where this one reaches 0.71 and the 64-row tiles of iou2d_kernel 0.68-0.69: the claims keep an image's write frontier
// compact when workgroups drift, and the workgroups that run out of units on their image finish the others'.)
// `claims`: one slot of the library's per-device claim ring (claim_ring_slot): [nimg] counters 64 ints apart, then an exit counter.  The
// slot is all zero when the launch starts, and the LAST workgroup to leave zeroes it again (device-scope exchanges, the path the claims
// themselves take) -- no memset in front of the launch and no allocation per call.
template <bool VEC>
__global__ __launch_bounds__(1024) void iou2d_self_kernel(const float* __restrict__ boxes, int N, int nimg, float* __restrict__ out, long ld,
                                                          int* __restrict__ claims) {
    writers_staged_2d<VEC>(boxes, N, out, ld, nimg, claims, 64, 0);      // (a counter per 256 bytes: each in an L2 line of its own)
    if (threadIdx.x == 0) {                                                 // (thread 0 issued every claim of this workgroup and has consumed them all)
        int* done = claims + (size_t)nimg * 64;
        if (atomicAdd(done, 1) == (int)gridDim.x - 1) {
            for (int i = 0; i <= nimg; ++i) atomicExch(claims + (size_t)i * 64, 0);
        }
    }
}

// LARGE images (N > 4096): the matrix write as a launch of its own on the side stream (3.2d), in the same geometry -- persistent
// workgroups of 16 waves, 8 rows x 256 columns per wave -- because that geometry is what the store stream likes: a plain fill written
// this way reaches 5.7-5.8 TB/s at N = 4096 ... 16384 where a linear grid-stride fill and gnms_iou2d's 64-row tiles reach 4.6-4.8
// (tools/kernel_times.py).  A unit = one row band (8 rows) of one column group (<= 16 wave tiles; the groups of an image are balanced) of one image, numbered
// (image, column group) major; every workgroup takes a contiguous range of them (no chain workgroup in this launch and nothing to
// balance, so no claims).  The column group's boxes are staged in LDS when the (image, group) changes; the row boxes of a workgroup's NEXT unit
// are loaded by wave 0 before the stores of the current one and parked in LDS after them (vmcnt(8), as the claim above).
template <bool VEC>
__global__ __launch_bounds__(1024) void write_staged_kernel(const float* __restrict__ A, const float* __restrict__ boxes, int M, int N, int nimg,
                                                            float* __restrict__ out, long ld) {
    using namespace gnms_iou;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sbox = reinterpret_cast<float4*>(smem);                  // [4096] column boxes of the staged (image, column group)
    float4* srow = sbox + 4096;                                      // [2][16] row boxes of the current / the next unit
    const float4* b4 = reinterpret_cast<const float4*>(boxes);        // columns: boxes [nimg][N][4]
    const float4* a4 = reinterpret_cast<const float4*>(A);            // rows: A [nimg][M][4] (the layer: the same boxes)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncc = (N + kWaveCols - 1) / kWaveCols;                 // wave tiles per row band
    const int ncg = (ncc + 15) >> 4;                                 // column groups ...
    const int tg = (ncc + ncg - 1) / ncg;                            // ... of tg <= 16 wave tiles each, balanced (17 tiles: 9 + 8, not 16 + 1)
    const int nb = (M + kStagedRows - 1) / kStagedRows;
    const long units = (long)nimg * ncg * nb;
    auto row_box = [&](long u, int r) {
        const long pair = u / nb;
        const int band = (int)(u - pair * nb), img = (int)(pair / ncg);
        return a4[(size_t)img * M + min(band * kStagedRows + r, M - 1)];
    };
    // a contiguous range of units per workgroup: at most a couple of stagings each, and 248 sequential store streams are what the
    // memory likes best (plain fill in this order: 5.5 / 6.0 / 5.9 TB/s at N = 4096 / 8192 / 16384)
    // (ranges of equal WORK, not of equal length: a unit of a ragged last column group keeps fewer than 16 waves busy and ends sooner)
    const int tlast = ncc - tg * (ncg - 1);                          // wave tiles in the last group
    const long wimg = (long)nb * ncc, wfull = (long)nb * tg;
    auto unit_of_work = [&](long s) {                                // the unit that holds tile-work offset s (units in (image, group) major order)
        const long img = s / wimg, rem = s - img * wimg;
        const long g = min((long)(ncg - 1), rem / wfull);
        const long band = (rem - g * wfull) / (g == ncg - 1 ? tlast : tg);
        return (img * ncg + g) * nb + band;
    };
    const long wtot = wimg * nimg;
    long u = unit_of_work(wtot * blockIdx.x / gridDim.x);
    const long uend = blockIdx.x + 1 == gridDim.x ? units : unit_of_work(wtot * (blockIdx.x + 1) / gridDim.x);
    if (u < uend && tid < kStagedRows) srow[tid] = row_box(u, tid);
    int ph = 0;
    long staged = -1;
    for (; u < uend; ++u) {
        const long pair = u / nb;
        const int band = (int)(u - pair * nb), img = (int)(pair / ncg), g = (int)(pair - (long)img * ncg);
        if (pair != staged) {                                        // (the barrier that ended the last unit covers the old contents)
            const int c0g = g * tg * kWaveCols, ncol = min(tg * kWaveCols, N - c0g);
            for (int i = tid; i < ncol; i += 1024) sbox[i] = b4[(size_t)img * N + c0g + i];
            staged = pair;
            __syncthreads();
        }
        const long un = u + 1;
        const bool fetch = tid < kStagedRows && un < uend;
        float4 nrow = make_float4(0.f, 0.f, 0.f, 0.f);
        const int c0 = (g * tg + wave) * kWaveCols;
        if (wave < tg && c0 < N)
            iou2d_tile_staged<VEC, kStagedRows>(sbox, g * tg * kWaveCols, srow + ph * kStagedRows, M, N, out + (size_t)img * M * ld, ld, band * kStagedRows, c0, lane,
                [&] { if (fetch) nrow = row_box(un, tid); },
                [&] { asm volatile("" :: "v"(nrow.x), "v"(nrow.y), "v"(nrow.z), "v"(nrow.w)); });
        if (fetch) srow[(ph ^ 1) * kStagedRows + tid] = nrow;
        __syncthreads();
        ph ^= 1;
    }
}

// the launch; reserve: CUs left without a writer workgroup for the layer's one-workgroup-per-image kernels on the caller's stream
int launch_write_staged(const float* a, const float* b, int B, int M, int N, float* out, int64_t ld, int reserve, hipStream_t st) {
    const int cus = gnms_device_cu_count();
    int grid = cus - reserve;
    if (grid < cus / 2) grid = cus / 2;
    const size_t lds = 96 * 1024;                                    // > 80 KiB: one writer workgroup per CU (it uses 4096 + 32 boxes = 64.5 KiB)
    int rc;
    if ((rc = allow_lds(write_staged_kernel<true>, lds))) return rc;
    gnms_launch_prof(kProfMatrixWrite, write_staged_kernel<true>, dim3((unsigned)grid), dim3(1024), lds, st, a, b, M, N, B, out, (long)ld);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
}  // namespace
// gnms_iou2d's large-matrix path (iou_kernels.hip): the persistent writers' geometry reaches 5.5-5.6 TB/s where its 64-row tiles reach 4.6-5.2
bool gnms_internal_iou2d_wants_staged(int B, int M, int N, int64_t ld, const float* out) {
    if ((ld % 4) != 0 || (N % 4) != 0 || ((uintptr_t)out % 16) != 0) return false;
    // (N <= 4096: the per-unit row fetch and barrier cost more than the geometry gains -- B = 8, M = N = 4096: 108-114 us against the
    // 64-row tiles' 102; N = 16384: 1.61 ms against 1.85)
    const long units = (long)B * ((M + kStagedRows - 1) / kStagedRows) * ((N + 4095) / 4096);
    return N > 4096 && units >= 4L * gnms_device_cu_count();
}
// a == b, N <= 4096: iou2d_self_kernel (B = 8, N = 4096: 0.68-0.69 -> 0.71 of the HBM peak)
bool gnms_internal_iou2d_wants_self(const float* a, const float* b, int B, int M, int N, int64_t ld, const float* out) {
    if (a != b || M != N || N > 4096 || B > 127) return false;
    const long units = (long)B * ((N + kStagedRows - 1) / kStagedRows) * ((N + 4095) / 4096);
    return units >= 8L * gnms_device_cu_count();
}
namespace {
// The claim counters of iou2d_self_kernel live in zeroed SLOTS of a per-device pool that the library allocates once (the first eager call on
// a device; 2 MiB) -- a launch leaves its slot zeroed (see the kernel), so a call neither allocates nor memsets.  Who may share a slot
// (a host-side round robin handed the same slot to launches that can run at the same time -- another stream, or a replayed graph
// that had the pointer baked in -- which then shared claim and exit counters and each wrote only part of its matrix):
//   * eager launches: ONE slot per (device, stream) -- launches of one stream run one after the other;
//   * a launch that is being CAPTURED: a slot of its own, never handed out again -- whatever the graph later runs beside, nobody else
//     counts in its slot (two replays of the same executable graph do not overlap);
//   * no slot left, or a capture before the pool exists (no allocation inside a capture): the caller falls back to iou2d_kernel.
// Images per call <= kClaimImgs (larger batches take iou2d_kernel).
constexpr int kClaimSlots = 64, kClaimImgs = 127;
constexpr size_t kClaimSlotInts = (size_t)(kClaimImgs + 1) * 64;
constexpr int kNoClaimSlot = 1;                                      // (> 0: not an error code)
int claim_slot_for(hipStream_t st, int** slot) {
    struct Pool { int* base = nullptr; int eager_next = 0, capture_next = kClaimSlots - 1; std::map<hipStream_t, int> by_stream; };
    static std::mutex mu;
    static std::map<int, Pool> pools;
    int dev = 0;
    GNMS_CHECK_HIP(hipGetDevice(&dev));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lock(mu);
    Pool& R = pools[dev];
    if (!R.base) {
        if (capturing) return kNoClaimSlot;
        int* p = nullptr;
        GNMS_CHECK_HIP(hipMalloc((void**)&p, kClaimSlots * kClaimSlotInts * sizeof(int)));
        const hipError_t e = hipMemset(p, 0, kClaimSlots * kClaimSlotInts * sizeof(int));
        if (e != hipSuccess) { (void)hipFree(p); GNMS_CHECK_HIP(e); }
        R.base = p;
    }
    // (the pool is finite: a slot per stream that ever called, one per captured launch, none reclaimed.  When it runs out the callers fall
    // back to their slower forms -- said once on stderr, so that the cliff is visible: ADVICE r5)
    auto exhausted = [] {
        static std::atomic<bool> said{false};
        if (!said.exchange(true))
            fprintf(stderr, "[groomed_nms_hip] all %d claim slots of this device are taken (one per stream that called, one per captured launch): "
                            "gnms_iou2d and the one-call entry on small images fall back to their slower kernels from here on\n", kClaimSlots);
        return kNoClaimSlot;
    };
    int idx;
    if (capturing) {
        if (R.capture_next < R.eager_next) return exhausted();
        idx = R.capture_next--;
    } else {
        auto it = R.by_stream.find(st);
        if (it != R.by_stream.end()) idx = it->second;
        else {
            if (R.eager_next > R.capture_next) return exhausted();
            idx = R.by_stream[st] = R.eager_next++;
        }
    }
    *slot = R.base + (size_t)idx * kClaimSlotInts;
    return GNMS_OK;
}
}  // namespace
// (returns 1 -- not an error -- when no claim slot is to be had: gnms_iou2d then runs iou2d_kernel)
int gnms_internal_iou2d_self(const float* boxes, int B, int N, float* out, int64_t ld, hipStream_t st) {
    const int cus = gnms_device_cu_count();
    int grid = cus - 8;                                              // (alone on the machine the stream likes every CU: 248 -> 0.71, 200 -> 0.64)
    if (grid < 1) grid = 1;
    int* claims = nullptr;
    int rc = claim_slot_for(st, &claims);
    if (rc) return rc;
    size_t lds = (size_t)N * 16;
    if (lds < 96 * 1024) lds = 96 * 1024;                            // > 80 KiB: one workgroup per CU
    const bool vec = (ld % 4 == 0) && ((uintptr_t)out % 16 == 0);
    if (vec) {
        if ((rc = allow_lds(iou2d_self_kernel<true>, lds))) return rc;
        gnms_launch_prof(kProfMatrixWrite, iou2d_self_kernel<true>, dim3((unsigned)grid), dim3(1024), lds, st, boxes, N, B, out, (long)ld, claims);
    } else {
        if ((rc = allow_lds(iou2d_self_kernel<false>, lds))) return rc;
        gnms_launch_prof(kProfMatrixWrite, iou2d_self_kernel<false>, dim3((unsigned)grid), dim3(1024), lds, st, boxes, N, B, out, (long)ld, claims);
    }
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
int gnms_internal_iou2d_staged(const float* a, const float* b, int B, int M, int N, float* out, int64_t ld, hipStream_t st) {
    return launch_write_staged(a, b, B, M, N, out, ld, 0, st);
}
namespace {

// gnms_forward_with_iou2d on small images as ONE launch (nms_one_launch.h): [matrix writers] [sort] [table from the boxes] [chain] [CSR].
// The writers are writers_staged_2d with a slot of the claim ring (as iou2d_self_kernel: zero at the start, re-zeroed by the last writer
// to leave).
__global__ __launch_bounds__(1024) void one_launch_boxes_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int N,
                                                                const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L,
                                                                float* __restrict__ prob, long long* __restrict__ valid, long long* __restrict__ invalid,
                                                                int* __restrict__ nvalid, int* __restrict__ ninvalid, long long* __restrict__ order_out,
                                                                int B, int kpw, int tpw, float* __restrict__ out, long ld, int* __restrict__ claims,
                                                                int nwriters) {
    GNMS_TINIT();
    // tpw == 0: the table with its sources in x order (one_launch_bits_from_boxes_x) -- [sort] [x sort] [table: NB a image] [chain] [CSR] [writers]:
    // two sort roles of B * nsort workgroups are a round of the machine by themselves, so the writers come LAST and start as the sorts retire
    const bool xt = tpw == 0;
    const int NP = (N + 63) & ~63, nsort = NP / kpw, nbits = xt ? L.NB : (L.NB * (L.NB + 1) / 2 + tpw - 1) / tpw;
    const int front = xt ? B * (2 * nsort + nbits + 2) : 0;
    int bx = (int)blockIdx.x, b;
    if (xt ? bx >= front : bx < nwriters) {
        // (rank-space table) the writers FIRST in the grid: they wait for nobody and are the longest role at N = 1024 (every workgroup of the launch holds a CU
        // to itself -- the chain's LDS -- so behind the sort and table workgroups they would only start when those retire: 36 us against 20)
        writers_staged_2d<true>(boxes, N, out, ld, B, claims, 64, front);
        if (threadIdx.x == 0) {                                             // (thread 0 issued every claim of this workgroup and has consumed them all)
            int* done = claims + (size_t)B * 64;
            if (atomicAdd(done, 1) == nwriters - 1) {
                for (int i = 0; i <= B; ++i) atomicExch(claims + (size_t)i * 64, 0);
            }
        }
        return;
    }
    if (xt) {
        if (bx < 2 * B * nsort) {
            const int role = bx >= B * nsort ? 1 : 0;
            bx -= role * B * nsort;
            b = bx / nsort;
            const unsigned tag = (unsigned)gnms_next_epoch(coh_load(img_ptrs(ws, L, b).misc + 8));
            if (kpw == 32) sort_count_body<32, true>(scores, boxes, N, counts, ws, L, order_out, 0, bx - b * nsort, b, role, tag);
            else sort_count_body<64, true>(scores, boxes, N, counts, ws, L, order_out, 0, bx - b * nsort, b, role, tag);
            return;
        }
        bx -= 2 * B * nsort;
        if (bx < B * nbits) {
            b = bx / nbits;
            const unsigned tag = (unsigned)gnms_next_epoch(coh_load(img_ptrs(ws, L, b).misc + 8));
            one_launch_bits_from_boxes_x(N, counts, P.nms_threshold, ws, L, b, bx - b * nbits, tag, nsort);
            return;
        }
        bx -= B * nbits;
        one_launch_chain_or_csr<kFromBoxes>(boxes, N, (long)N, counts, P, ws, L, prob, valid, invalid, nvalid, ninvalid, B, bx, nsort, nbits);
        return;
    }
    bx -= nwriters;
    if (bx < B * nsort) {
        b = bx / nsort;
        const unsigned tag = (unsigned)gnms_next_epoch(coh_load(img_ptrs(ws, L, b).misc + 8));
        if (kpw == 32) sort_count_body<32, true>(scores, boxes, N, counts, ws, L, order_out, 0, bx - b * nsort, b, 0, tag);
        else sort_count_body<64, true>(scores, boxes, N, counts, ws, L, order_out, 0, bx - b * nsort, b, 0, tag);
        return;
    }
    bx -= B * nsort;
    if (bx < B * nbits) {
        b = bx / nbits;
        const unsigned tag = (unsigned)gnms_next_epoch(coh_load(img_ptrs(ws, L, b).misc + 8));
        one_launch_bits_from_boxes(N, counts, P.nms_threshold, ws, L, b, bx - b * nbits, tpw, tag, nsort);
        return;
    }
    bx -= B * nbits;
    one_launch_chain_or_csr<kFromBoxes>(boxes, N, (long)N, counts, P, ws, L, prob, valid, invalid, nvalid, ninvalid, B, bx, nsort, nbits);
}

}  // namespace

// bitmask_boxes_kernel: workgroups of 4 wave tiles, (row blocks) x (column chunks) tiles per image; 4 columns per lane
// (64 x 256 tiles) when that already gives every SIMD a couple of waves, else 1 column per lane (64 x 64 tiles)
int gnms_internal_launch_bitmask_boxes(const LayerCall& c, const float* boxes) {
    const int B = c.B, N = c.N;
    const gnms_ws_layout& L = c.L;
    const int NB = (N + 63) / 64;
    const long long tiles4 = (long long)B * NB * ((N + 255) / 256);
    const int wt = w_write_through_routes();
    if (N > 4096 && N % 1024 == 0) {
        // large images (round 4b): the scatter kernel with the row groups dealt to the XCDs (bitmask_boxes_pinned_kernel) -- a row of W is
        // >= 64 KiB here and completing its lines in ONE L2 costs less than collecting it in LDS first (one 16-wave workgroup per CU):
        // B = 8, N = 16384 280 -> 189 us (step 1.74 -> 1.66 ms), 8192 82 -> 61.  Row groups of 4 blocks where there are plenty of tiles
        // (16384: 288 / 217 / 189 / 184 us with 1 / 2 / 4 / 8).
        const int kbw = tiles4 >= 32768 ? 4 : 1;
        const unsigned gx = (unsigned)(gnms_div_up(gnms_div_up(NB, kbw), 8) * (((N + 255) / 256) / 4) * 8);
        if (kbw >= 4) bitmask_boxes_pinned_kernel<4><<<dim3(gx, 1, B), 256, 0, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L);
        else bitmask_boxes_pinned_kernel<1><<<dim3(gx, 1, B), 256, 0, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L);
    } else if (tiles4 >= 32768) {
        // large images (round 3): the LDS row buffer with a chunk loop -- one 16-wave workgroup per rank block, its waves walking the
        // column chunks, the full row of W leaving as ONE coalesced write (N <= GNMS_MAX_BOXES: the row fits 128 KiB).  The scatter
        // kernel it replaced issued N^2 / 64 scattered 8-byte stores per image: B = 8, N = 16384 step 1.907 -> 1.798 ms.
        const size_t lds = (size_t)L.NC * 8;
        int rc = allow_lds(bitmask_boxes_kernel<4, 1, true, true>, lds);
        if (rc) return rc;
        bitmask_boxes_kernel<4, 1, true, true><<<dim3(NB, 1, B), 1024, lds, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L, wt & kWtChunkLoop);
    } else if (tiles4 >= 2048 && (N + 255) / 256 <= 16) {
        // one 16-wave workgroup per rank block: words collected in an LDS copy of the row, written out coalesced
        // (from two workgroups per CU on: two rank blocks per workgroup -- half the column-side traffic, one workgroup per CU; see the body)
        if ((long)B * NB > (long)gnms_device_cu_count()) {
            const size_t lds = 2 * (size_t)L.NC * 8;                   // (the ranks stay in registers here: no stash)
            int rc = allow_lds(bitmask_boxes_kernel<4, 2, true>, lds);
            if (rc) return rc;
            bitmask_boxes_kernel<4, 2, true><<<dim3((NB + 1) / 2, 1, B), 1024, lds, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L, wt & kWtKbw2);
        } else
        bitmask_boxes_kernel<4, 1, true><<<dim3(NB, 1, B), 1024, (size_t)L.NC * 8 + 4 * 1024 * sizeof(int), c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L, wt & kWtKbw1);   // + the ranks' stash
    } else if (tiles4 >= 2048) {
        bitmask_boxes_kernel<4, 1><<<dim3(gnms_div_up(NB * ((N + 255) / 256), 4), 1, B), 256, 0, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L, 0);
    } else {
        bitmask_boxes_kernel<1, 1><<<dim3(gnms_div_up(NB * NB, 4), 1, B), 256, 0, c.st>>>(boxes, N, c.counts, c.P.nms_threshold, c.ws, L, 0);
    }
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

namespace {
// GNMS_RANK_SORT=0: 2048 < N <= 4096 sorts as runs + merge, two launches (developer / test switch, read once: the pair stays reachable for
// A/B runs and the tests)
bool rank_sort_enabled() { static const bool on = env_switch("GNMS_RANK_SORT", 1) != 0; return on; }
// GNMS_HIST_SORT=0: the routing of round 8, no histogram sort (the same kind of switch)
bool hist_sort_enabled() { static const bool on = env_switch("GNMS_HIST_SORT", 1) != 0; return on; }
}  // namespace
// keys in one bin from which on sort_hist_rank_kernel falls back to the run sort; gnms_profile_set_hist_cap moves it for the cap series
std::atomic<int>& gnms_internal_hist_cap() { static std::atomic<int> cap{kHistCap}; return cap; }

// K1: stable descending score sort (+ the x-centre sort of the boxes when `boxes` is given).  Which kernels (measured per call in a replayed
// graph of 20, MI355X, LABNOTES R8.1 and R13.3; G = workgroups of the counting sort = N / 64 * B * roles, W = workgroups of the one-launch sorts
// of 2048 < N <= 4096 = 16 * B * roles):
//   N <= 2048; N <= 4096 with G <= CUs / 2 (N = 4096: B = 1 with boxes, B <= 2 without)   by counting, one launch (sort_count_kernel)
//   2048 < N <= 4096 otherwise, while W <= 3 CUs (B <= 24 with boxes, 48 without)       by histogram, one launch (sort_hist_rank_kernel, round 13)
//   everything else (N > 4096; W > 3 CUs; GNMS_RANK_SORT=0)                             runs of 1024 + rank merge, two launches
// GNMS_HIST_SORT=0 is the table of round 8: counting up to G <= CUs, then 16 wave-sorted runs per workgroup ranked in the same launch
// (sort_ranked_runs_kernel) while W <= CUs, then runs + merge.
// N = 4096, us per call, by histogram / ranked runs / runs + merge / counting: with boxes B = 1 7.45 / 9.8 / 12.4 / 7.42 (counting keeps it), B = 2
// 7.5 / 10.0 / 12.4 / 10.0, B = 4 7.7 / 10.4 / 12.8, B = 8 8.0 / 11.5 / 13.4, B = 16 (two rounds of the machine) 10.7 / 16.3 / 15.0, B = 24 14.6 / 22.2 /
// 16.4, B = 32 18.1 / 27.0 / 18.0 (runs + merge from here); scores alone B = 2 7.1 / 9.1 / 12.1 / 6.7 (counting), B = 4 7.2 / 9.3 / 12.2 / 9.3, B = 8
// 7.4 / 9.6 / 12.4, B = 16 7.7 / 10.3 / 12.7, B = 32 10.4 / 15.2 / 13.9, B = 64 17.6 / 25.3 / 16.4; N = 2112 with boxes B = 2 6.3 / 9.3 / 12.1 / 6.6,
// B = 3 6.4 / 9.4 / 12.3 / 6.8, B = 8 6.7 / 10.1 / 12.6; N = 3072 B = 8 7.4 / 10.6 / 13.2.
// mode3d: 0 = `boxes` are 2D boxes (columns by x centre); >= 1 = pseudo boxes of cuboids whose records lie in the workspace (columns by
// (z band, x centre) with that many bands; the sort also leaves the records in column order, ImgPtrs::xrec)
// route (gnms_profile_sorts): 0 = the table above, 1 = runs + merge, 2 = ranked runs, 3 = by histogram
int gnms_internal_launch_sorts(const LayerCall& c, const float* scores, const float* boxes, int mode3d, int route) {
    const int B = c.B, N = c.N, P2 = c.P2;
    int rc;
    const int roles = boxes ? 2 : 1;
    const long cus = (long)gnms_device_cu_count();
    const long one_launch_wgs = (long)kRankRuns * B * roles;
    const bool one_launch = P2 == 4096 && rank_sort_enabled();
    const bool hist = one_launch && hist_sort_enabled() && one_launch_wgs <= 3 * cus;
    // up to 2048 keys: by counting, N / 64 workgroups per image and role (sort_count_kernel)
    // (... and up to 4096 keys while those workgroups fill at most half the machine, 256 compares per thread; on a full round the count takes
    // 9.3-10.0 us and the histogram sort 7.2-7.5.  Without the histogram sort: while they are one round, level with the ranked runs, LABNOTES R5.6)
    const long count_wgs = (long)B * ((N + 63) / 64) * roles;
    if (route == 0 && (N <= 2048 || (N <= 4096 && (hist ? 2 * count_wgs : count_wgs) <= cus))) {
        const int NP = (N + 63) & ~63;
        if (NP % 128 == 0 && (long)B * (NP / 32) * roles <= cus)        // half the compares per thread while the grid is one round
            sort_count_kernel<32><<<dim3(NP / 32, B, roles), 1024, (size_t)NP * 8, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, (long long*)c.order, mode3d);
        else
            sort_count_kernel<64><<<dim3(NP / 64, B, roles), 1024, (size_t)NP * 8, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, (long long*)c.order, mode3d);
        GNMS_CHECK_LAUNCH();
        return GNMS_OK;
    }
    // 2048 < N <= 4096 past that: one launch, 16 workgroups per image and role, each holding all keys of its image.  By histogram no workgroup
    // sorts anything, and a second and third round of the machine still beat the second launch of runs + merge; the ranked runs repeat the
    // image's run sort in every workgroup and are taken only while they are one round.
    if (route == 2 || route == 3 || (route == 0 && one_launch && (hist || one_launch_wgs <= cus))) {
        if (P2 != 4096) {
            gnms_set_error("launch_sorts: the %s sort takes 2048 < N <= 4096 (N=%d)", route == 3 ? "histogram" : "ranked-runs", N);
            return GNMS_ERR_UNSUPPORTED;
        }
        const dim3 grid(kRankRuns, B, roles);
        const size_t lds = (size_t)kRankRuns * kRankRunKeys * 8;
        if (route == 3 || (route == 0 && hist))
            sort_hist_rank_kernel<<<grid, 1024, lds, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, (long long*)c.order, mode3d, gnms_internal_hist_cap().load());
        else
            sort_ranked_runs_kernel<<<grid, 1024, lds, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, (long long*)c.order, mode3d);
        GNMS_CHECK_LAUNCH();
        return GNMS_OK;
    }
    if (P2 <= 1024) {
        sort_scores_kernel<1><<<dim3(B, roles), P2, (size_t)P2 * 8, c.st>>>(scores, N, c.counts, c.ws, c.L, P2, (long long*)c.order, boxes, mode3d);
        GNMS_CHECK_LAUNCH();
        return GNMS_OK;
    }
    const int R = P2 / 1024;
    const size_t lds = (size_t)P2 * 8;
    // (runs and merge as ONE launch with nonce-flag hand-offs was measured in round 3: 13.1 us against 7.8 + 6.2, the step unchanged -- a launch
    // boundary between two small kernels costs ~1 us; dropped in round 4, LABNOTES.md)
    sort_runs_kernel<<<dim3(R, B, roles), 1024, 0, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, P2, mode3d);
    GNMS_CHECK_LAUNCH();
#define GNMS_MERGE(RR)                                                                                                    \
    do {                                                                                                                  \
        if ((rc = allow_lds(sort_merge_kernel<RR>, lds))) return rc;                                                      \
        sort_merge_kernel<RR><<<dim3(RR, B, roles), 1024, lds, c.st>>>(scores, boxes, N, c.counts, c.ws, c.L, (long long*)c.order, mode3d); \
    } while (0)
    switch (R) {
        case 2: GNMS_MERGE(2); break;
        case 4: GNMS_MERGE(4); break;
        case 8: GNMS_MERGE(8); break;
        default: GNMS_MERGE(16); break;
    }
#undef GNMS_MERGE
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

// 3D: the write role of the tail launch as symmetric writers (writers_sym_persistent) -- above N = 1024, where an image has enough
// macro tiles.
bool gnms::sym_writers_in_tail_launch(int N, int64_t ld, const float* out) {
    if (!gnms_internal_overlap3d_sym_ok(N, ld, out)) return false;
    return N > 1024;                                              // (B = 8: N = 2048 0.110 -> 0.090 ms, 1536 0.0895 -> 0.080, 1024 even)
}

// A small image's whole forward pass as ONE launch (nms_one_launch.h): masked groups, hard sort, N <= 1024 (one super-block), a 16-byte
// aligned matrix with ld % 4 == 0, and no more workgroups than two rounds of the machine (every one asks for the chain's LDS, so a CU
// holds one).  GNMS_ONE_LAUNCH=0: never (developer / test switch: the three-launch path stays reachable for A/B runs and the tests).
bool gnms::one_launch_enabled() { static const bool on = env_switch("GNMS_ONE_LAUNCH", 1) != 0; return on; }

namespace {

// K3..K6 as one launch or four?  Measured (HIP-graph replay, B=8): one launch wins 2-2.5 us per step up to N=2048 (three
// kernel boundaries less) and, with the general scan, loses 1.5 us at N=4096 (the attribution runs on one CU instead of 64).  Where the
// scan attributes as it goes (symmetric sources, `sym`), K4 rides in K5 and K6 starts from LDS (groups_body FUSE, E <= 4): one launch
// up to N = 4096.
bool use_tail_kernel(int N, int sym = 0) {
    return N <= 2048 || (sym && N <= 4096);
}

// chain workgroups per image when the matrix write runs beside the layer as a launch of its own on the side stream (N > 4096): ONE, which
// walks the image's super-blocks in order.  The write there is a static partition over (CUs - reserve) persistent workgroups and takes
// 1.45 ms at B = 8, N = 16384; the scan of a whole image on one CU (~1 ms beside it) hides behind that, while every further chain
// workgroup either costs the write a CU (32 reserved: write 1.52 ms, step 1.86) or, unreserved, does not find a CU before the writers
// retire and stalls the chain behind the write (16 per image, 8 reserved: step 1.82 against 1.74).
constexpr int kBesideChainWGs = 1;

// the one launch of a small image (one_launch_enabled above)
struct OneLaunchPlan { bool ok; int kpw, tpw, split; long front; };   // front: the launch's workgroups without the matrix writers
// keys per sort workgroup with the x-order table: 64.  (Measured: 128 keys a workgroup -- two sort roles + the tables then fit one round of the
// machine, so every table workgroup is resident from the start -- loses to the longer count: B = 8 N = 1024 31.0 against 29.7 us, B = 8 N = 768
// 27.4 / 26.6, B = 4 N = 1024 30.3 / 29.1; 32 keys where that fits half the machine: B = 2 N = 1024 28.0 / 28.2 -- no difference.)
constexpr int kXtKpw = 64;
// The geometry of the one launch, for the layer from the matrix (gnms_forward: src = kFromMatrix) and for the one-call entry
// (gnms_forward_with_iou2d: src = kFromBoxes), and whether the call takes it at all -- the pointers' alignment apart, which the launchers look at.
OneLaunchPlan one_launch_plan(int src, int B, int N, const gnms_params& P) {
    OneLaunchPlan p = {false, 0, 0, 0, 0};
    if (!one_launch_enabled() || !fast_tail_enabled() || N > kOneLaunchMaxN || !fast_tail_ok(N, P, 1)) return p;
    const int cus = gnms_device_cu_count();
    const int NP = (N + 63) & ~63, NB = NP / 64, nbp = NB * (NB + 1) / 2;
    p.kpw = (NP % 128 == 0 && (long)B * (NP / 32) <= (long)cus / 2) ? 32 : 64;
    if (src == kFromMatrix) {
        p.split = 4;                                              // table workgroups: 16 rows each while that leaves the machine half empty
        while (p.split > 1 && (long)B * NB * p.split > (long)cus / 2) p.split >>= 1;
        p.front = (long)B * (NP / p.kpw + NB * p.split + 2);
        p.ok = p.front <= 2L * cus;
        return p;
    }
    if (B > kClaimImgs) return p;
    // which table the one-call entry's one launch builds: rank space (tpw = 1: one 64 x 64 task per workgroup, while all tasks are at most one
    // round of the machine), sources in x order (tpw = 0: beyond that, while the launch's front is at most two rounds), or none (three launches)
    // One task (a 64 x 64 block of pair decisions on 16 waves) per table workgroup, and only while all of them are about one round of the
    // machine: in rank space nothing can be culled, and where the tasks queue the three launches (x-sorted, culled bit matrix: 5-7 us) win.
    // Kernel time of the launch against sort + bits + tail_write_kernel, us (profiles/r06g_*): B = 8 N = 256 18.3 / 25.0, B = 16 N = 256
    // 17.5 / 24.9, B = 1 / 2 N = 500 18.1 / 20.5 and 18.2 / 21.9, B = 8 N = 512 22.8 / 23.4, B = 1 N = 1024 23.4 / 25.1 -- and with 2 / 4 / 8
    // tasks per workgroup B = 2 / 4 / 8 at N = 1024: 28.0 / 25.9, 31.2 / 26.7, 37.9 / 33.5 (the one launch loses).
    // Beyond one round: the table with its SOURCES IN X ORDER (one_launch_bits_from_boxes_x, tpw = 0) -- NB culled workgroups a image instead of
    // NB (NB + 1) / 2 unculled ones, for a second sort role (the boxes by x centre) in the launch and the writers behind everything.  Kernel
    // time, x-order table / rank-space table or the three launches, us, same box (profiles/r06x_*): B = 8 N = 1024 31.3 / 35.2 (three launches),
    // B = 4 N = 1024 29.8 / 32.0, B = 16 N = 512 24.1 / 29.0, B = 8 N = 768 27.6 / 32.5, B = 4 N = 768 25.8 / 27.3, B = 2 N = 1024 28.9 / 31.1,
    // B = 8 N = 512 24.4 / 25.9 -- and below a round of tasks the rank-space table wins: B = 1 N = 1024 27.1 / 25.0, B = 4 N = 512 23.2 / 20.2,
    // B = 16 N = 256 21.9 / 18.8, B = 8 N = 256 22.0 / 18.3, B = 1, 2 N = 500 21.8 / 19.4, 22.5 / 19.6.
    if ((long)B * nbp <= (long)cus && nbp <= 13 * 32) {
        p.tpw = 1;
        p.front = (long)B * (NP / p.kpw + nbp + 2);
        p.ok = p.front <= 3L * cus;
    } else {
        p.kpw = kXtKpw;
        p.tpw = 0;
        p.front = (long)B * (2 * (NP / kXtKpw) + NB + 2);
        p.ok = p.front <= 2L * cus;
    }
    return p;
}
// The one launch zeroes nothing of the workspace: its roles hand over through granules that carry tag = next(misc[8]).  A recycled workspace
// can hold an EARLIER call's granules beside a counter that something else has overwritten since (another tensor of the caching allocator,
// an allocation of the same captured graph) -- then the new tag can equal the stale granules' and a role goes ahead on the previous call's
// data (seen: csr_build_body built the backward's runs from the last call's heads; the probabilities were right, dL/dscores was not).
// So the granules of every image are cleared in front of the launch, stream-ordered: a cleared granule carries tag 0, which no call uses.
__global__ __launch_bounds__(256) void clear_granules_kernel(char* ws, gnms_ws_layout L) {
    u64* g = reinterpret_cast<u64*>(ws + (size_t)blockIdx.x * L.per_image + L.off_gran);
    for (int i = threadIdx.x; i < 17 * 32; i += 256) g[i] = 0ull;
}
int clear_granules(const LayerCall& c) {
    clear_granules_kernel<<<c.B, 256, 0, c.st>>>(c.ws, c.L);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
// (both launchers: *launched stays false where the call does not take the one launch)
int launch_one_matrix(const LayerCall& c, const float* scores, const float* iou, int64_t ld, bool* launched) {
    *launched = false;
    if (!((ld % 4 == 0) && ((uintptr_t)iou % 16 == 0))) return GNMS_OK;
    const OneLaunchPlan plan = one_launch_plan(kFromMatrix, c.B, c.N, c.P);
    if (!plan.ok) return GNMS_OK;
    const size_t lds = one_launch_lds_size(c.N, false);
    int rc;
    if ((rc = allow_lds(one_launch_kernel<kFromMatrix>, lds))) return rc;
    if ((rc = clear_granules(c))) return rc;
    // (profile slot of the matrix READ: this launch holds the layer's one pass over the matrix -- bench.py's `roofline_matrix_in`)
    gnms_launch_prof(kProfMatrixRead, one_launch_kernel<kFromMatrix>, dim3((unsigned)plan.front), dim3(1024), lds, c.st, scores, iou, c.N, (long)ld, c.counts, c.P, c.ws, c.L,
                     c.prob, (long long*)c.valid, (long long*)c.invalid, c.nvalid, c.ninvalid, (long long*)c.order, c.B, plan.kpw, plan.split);
    GNMS_CHECK_LAUNCH();
    *launched = true;
    return GNMS_OK;
}

// the one-call entry (gnms_forward_with_iou2d, masked groups): the same with the table from the boxes and the matrix writers behind the chain
int launch_one_boxes(const LayerCall& c, const float* scores, const float* boxes, float* out, int64_t ld, bool* launched) {
    *launched = false;
    if (!((ld % 4 == 0) && ((uintptr_t)out % 16 == 0))) return GNMS_OK;
    const OneLaunchPlan plan = one_launch_plan(kFromBoxes, c.B, c.N, c.P);
    if (!plan.ok) return GNMS_OK;
    const int B = c.B, N = c.N, cus = gnms_device_cu_count();
    const bool xt = plan.tpw == 0;
    int* claims = nullptr;
    int rc = claim_slot_for(c.st, &claims);
    if (rc == kNoClaimSlot) return GNMS_OK;
    if (rc) return rc;
    const int ncc = (N + gnms_iou::kWaveCols - 1) / gnms_iou::kWaveCols, nrt = (N + kStagedRows - 1) / kStagedRows;
    long writers = (long)B * ((ncc * nrt + 15) >> 4);
    // (3/8 of the CUs write: at ~29 GB/s per writer workgroup the 32 MB of B = 8, N = 1024 then take as long as sort -> table -> chain
    // beside them on the other 5/8)
    const long cap = xt ? (long)cus / 2 : (long)cus * 3 / 8;                 // (x-order table: the writers are last in the grid and start as the sorts retire)
    if (writers > cap) writers = cap;
    if (writers < 1) writers = 1;
    size_t lds = one_launch_lds_size(N, true);
    if (lds < (size_t)N * 16) lds = (size_t)N * 16;
    if ((rc = allow_lds(one_launch_boxes_kernel, lds))) return rc;
    if ((rc = clear_granules(c))) return rc;
    gnms_launch_prof(kProfMatrixWrite, one_launch_boxes_kernel, dim3((unsigned)(plan.front + writers)), dim3(1024), lds, c.st, scores, boxes, N, c.counts, c.P, c.ws, c.L,
                     c.prob, (long long*)c.valid, (long long*)c.invalid, c.nvalid, c.ninvalid, (long long*)c.order, B, plan.kpw, plan.tpw, out, (long)ld, claims,
                     (int)writers);
    GNMS_CHECK_LAUNCH();
    *launched = true;
    return GNMS_OK;
}

// the layer from the matrix.  boxes2d: the 2D boxes `iou` was computed from (gnms_forward_with_iou2d), 16-byte aligned, or null: the
// ungrouped mode then builds its pruned lower-triangular matrix from them instead of reading `iou` back
int forward_matrix(const LayerCall& c, const float* scores, const float* iou, int64_t ld, const float* boxes2d = nullptr) {
    const int B = c.B, N = c.N;
    const gnms_params& P = c.P;
    int rc;
    bool launched = false;                                        // a small image: sort, threshold bits and chain as one launch
    if ((rc = launch_one_matrix(c, scores, iou, ld, &launched)) || launched) return rc;
    const bool permute_from_boxes = boxes2d && !P.group_boxes && !P.presorted;
    // (with the boxes the score sort also leaves them in rank order, rbox; its second role, the boxes by x centre, is not used here)
    if ((rc = gnms_internal_launch_sorts(c, scores, permute_from_boxes ? boxes2d : nullptr))) return rc;

    if (masked_groups(P) && use_tail_kernel(N, matrix_sym_detection(N) ? 2 : 0)) {
        // (with the fast tail the symmetry check is a role of the tail launch and the scan runs on trust beside it: sym 3)
        const int sym = matrix_sym_detection(N) ? ((fast_tail_enabled() && fast_tail_ok(N, P, 2)) ? 3 : 2) : 0;
        if ((rc = gnms_internal_launch_bitmask(c, iou, ld, sym == 3 ? 2 : (sym ? 1 : 0)))) return rc;
        return gnms_internal_launch_tail<kFromMatrix>(c, iou, ld, sym);
    }
    if (P.group_boxes) {
        const int sym = matrix_sym_detection(N) ? 2 : 0;
        if ((rc = gnms_internal_launch_bitmask(c, iou, ld, sym ? 1 : 0))) return rc;
        return launch_separate_tail<kFromMatrix>(c, iou, ld, sym);
    }
    float* Ps = reinterpret_cast<float*>(c.ws + (size_t)B * c.L.per_image);      // scratch behind the per-image regions
    const size_t plds = (size_t)N * 4;
    if ((rc = allow_lds(ungrouped_permute_kernel, plds))) return rc;
    ungrouped_prepare_kernel<<<dim3(gnms_div_up(N, 1024), B), 1024, 0, c.st>>>(N, c.counts, P, c.ws, c.L);
    GNMS_CHECK_LAUNCH();
    if (permute_from_boxes) ungrouped_permute_boxes_kernel<<<dim3(gnms_div_up(N, kPermuteRows), B), 256, 0, c.st>>>(N, c.counts, P, c.ws, c.L, Ps);
    else ungrouped_permute_kernel<<<dim3(N, B), 256, plds, c.st>>>(iou, N, (long)ld, c.counts, P, c.ws, c.L, Ps);
    GNMS_CHECK_LAUNCH();
    if ((rc = allow_lds(ungrouped_solve_forward_kernel, kUngroupedFwdLds))) return rc;
    ungrouped_solve_forward_kernel<<<dim3(gnms_div_up(N, kUB), B), kUThreads, kUngroupedFwdLds, c.st>>>(scores, N, c.counts, P, c.ws, c.L, Ps);
    GNMS_CHECK_LAUNCH();
    return launch_finalize(c);
}

}  // namespace

extern "C" int gnms_forward(const float* scores, const float* iou, int B, int N, int64_t ld, const int32_t* counts,
                            const gnms_params* params, float* prob, int64_t* order, int64_t* valid, int64_t* invalid,
                            int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes, void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_forward", &c, B, N, ld, counts, params, workspace, workspace_bytes, stream, false, scores && iou && prob,
                    "gnms_forward: null scores/iou/prob", prob, order, valid, invalid, nvalid, ninvalid);
    return forward_matrix(c, scores, iou, ld);
}

namespace {
// Large images (N > 4096, matrix >= 384 MiB): the matrix write takes longer than the layer behind it and nothing in the masked
// from-boxes layer reads it, so the write goes to a library-owned second stream and the layer's own kernels run beside it on the
// caller's stream.  A fork and a join cost 7-25 us of idle queue each and the layer's latency-bound kernels run 1.3-3x slower
// beside the write, which is why smaller problems stay on one stream (B=8, N=4096: 0.180-0.187 against 0.193 ms, not worth a
// second code path; B=4: 0.152 against 0.138; N=8192, B=1: even; B=2: 0.246 against 0.306).
struct SideStream { hipStream_t s = nullptr; hipEvent_t fork[2] = {nullptr, nullptr}, join = nullptr; };
std::mutex g_side_mu;
bool use_side_stream(int B, int N, int64_t ld) {
    return N > 4096 && (long long)B * N * ld * 4 >= (384ll << 20);
}
// the caller holds g_side_mu
int side_stream(SideStream** out) {
    static std::map<int, SideStream> per_dev;
    int dev = 0;
    GNMS_CHECK_HIP(hipGetDevice(&dev));
    SideStream& S = per_dev[dev];
    if (!S.s) {
        hipStream_t s = nullptr;
        // lowest priority: the write's workgroups fill every CU, and the layer's kernels on the caller's stream (some of them one
        // 128-KiB-LDS workgroup per image) must get the CU slots that free up, not wait for the write to drain
        int least = 0, greatest = 0;
        GNMS_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        GNMS_CHECK_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least));
        GNMS_CHECK_HIP(hipEventCreateWithFlags(&S.fork[0], hipEventDisableTiming));
        GNMS_CHECK_HIP(hipEventCreateWithFlags(&S.fork[1], hipEventDisableTiming));
        GNMS_CHECK_HIP(hipEventCreateWithFlags(&S.join, hipEventDisableTiming));
        S.s = s;
    }
    *out = &S;
    return GNMS_OK;
}
// everything enqueued on `st` so far happens before what is enqueued on the side stream from now on (`which`: a call that
// forks twice uses a different event each time)
int side_fork(hipStream_t st, hipStream_t* side, int which = 0) {
    std::lock_guard<std::mutex> lock(g_side_mu);
    SideStream* S = nullptr;
    int rc = side_stream(&S);
    if (rc) return rc;
    GNMS_CHECK_HIP(hipEventRecord(S->fork[which], st));
    GNMS_CHECK_HIP(hipStreamWaitEvent(S->s, S->fork[which], 0));
    *side = S->s;
    return GNMS_OK;
}
// the matrix write that gnms_forward_with_iou2d hands to the from-boxes layer for the side stream
struct MatrixWrite { float* out; int64_t ld; bool one_launch; };   // one_launch: inside the chain's launch (tail_write_kernel), else on the side stream
// The write in two launches: rows [0, r) beside the bit-matrix kernel (a VALU-bound kernel of small workgroups, which interleaves
// with the write's), the rest beside the tail.  r as a percentage of N (GNMS_SPLIT_PCT overrides), rounded down to whole 64-row
// tiles.  Measured B=8: 2D N=8192 0.625 / 0.575 / 0.568 / 0.595 ms at 0 / 20 / 40 / 50 %, N=16384 2.10 / 2.03 / 2.08 / 2.08;
// 3D N=8192 0.720 / 0.672 / 0.676 / 0.703, N=16384 2.39 / 2.37 / 2.36 / 2.36 (its write kernel has less VALU to spare).
int split_rows(int N, int pct) { return (int)((long long)N * pct / 100) & ~63; }
// everything enqueued on the side stream so far happens before what is enqueued on `st` from now on
int side_join(hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_side_mu);
    SideStream* S = nullptr;
    int rc = side_stream(&S);
    if (rc) return rc;
    GNMS_CHECK_HIP(hipEventRecord(S->join, S->s));
    GNMS_CHECK_HIP(hipStreamWaitEvent(st, S->join, 0));
    return GNMS_OK;
}
// fork(s) and the one join of a call; the destructor joins on an early (error) return, so that the caller's stream always
// covers what was put on the side stream
struct SideScope {
    hipStream_t st;
    bool forked = false;
    explicit SideScope(hipStream_t s) : st(s) {}
    ~SideScope() { if (forked) side_join(st); }
    int fork(hipStream_t* side, int which) { const int rc = side_fork(st, side, which); if (!rc) forked = true; return rc; }
    int join() { forked = false; return side_join(st); }
};
}  // namespace

namespace {
int forward_boxes(const LayerCall& c, const float* boxes, const float* scores, const MatrixWrite* mw = nullptr);

// Where the 3D entry's matrix is written (masked hard-sorted groups): in_tail -- K3..K6 and the matrix in one launch (tail_write_kernel), like
// the 2D entry; beside -- on the side stream; neither -- a launch of its own in front of the layer.
struct Write3dRoute { bool in_tail, beside; };
Write3dRoute write3d_route(int B, int N, int64_t ld, const float* out, float thr) {
    const bool culled_bits = thr >= 0.01f && thr < INFINITY;         // the culled bit-matrix kernel writes full symmetric rows of W
    // 1024 < N, no side stream: K3..K6 ride in the launch of the SYMMETRIC writers (tail_write_kernel, writers_sym_persistent) behind
    // the from-records bit-matrix kernel
    const bool sym_tail = culled_bits && sym_writers_in_tail_launch(N, ld, out);
    const bool beside = !sym_tail && use_side_stream(B, N, ld);
    // K3..K6 inside the write launch like the 2D entry -- up to N = 2048 only: the 3D writers are VALU-bound (23 slots per pair) and
    // at the one workgroup per CU that launch runs at they lose more than the overlap buys (B = 8, N = 4096: launch 166 us against a
    // 107-us write + 55-us chain, step 0.264 against 0.248 ms; N = 2048: 0.117 against 0.163 ms)
    return Write3dRoute{!beside && culled_bits && (N <= 2048 || sym_tail), beside};
}
}  // namespace

// name, as a kernel trace lists it, of the launch that writes the matrix inside gnms_forward_with_iou2d (dim 2) / _iou3d (dim 3)
// (default parameters, aligned inputs): the entries' own route decisions, asked for such a call
extern "C" const char* gnms_profile_write_kernel_name(int dim, int B, int N) {
    if (B <= 0 || N <= 0) return "";
    gnms_params P;
    gnms_default_params(&P);
    if (dim == 3) return write3d_route(B, N, N, nullptr, P.nms_threshold).in_tail ? "tail_write_kernel" : "iou3d_nms_fast_kernel";
    if (use_side_stream(B, N, N)) return N % 4 == 0 ? "write_staged_kernel" : "iou2d_kernel";
    return one_launch_plan(kFromBoxes, B, N, P).ok ? "one_launch_boxes_kernel" : "tail_write_kernel";
}

// The matrix is an OUTPUT here, so the layer does not have to read it back: with the boxes at hand the grouped modes
// take their threshold bits and the few P[i, head] entries straight from the boxes (bit-identical arithmetic, the
// from-boxes kernels), which replaces the 537 MB read of bitmask_kernel (~100 us at B=8, N=4096) by bitmask_boxes_kernel
// (~25 us, compute bound).  The ungrouped / soft-sorted modes read the matrix they just wrote.
extern "C" int gnms_forward_with_iou2d(const float* boxes, const float* scores, int B, int N, int64_t ld, const int32_t* counts,
                                       const gnms_params* params, float* iou_out, float* prob, int64_t* order, int64_t* valid,
                                       int64_t* invalid, int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_forward_with_iou2d", &c, B, N, ld, counts, params, workspace, workspace_bytes, stream, false,
                    boxes && scores && iou_out && prob, "gnms_forward_with_iou2d: null pointer", prob, order, valid, invalid, nvalid, ninvalid);
    const gnms_params& P = c.P;
    const bool from_boxes = from_boxes_2d(P, boxes);
    const bool beside = from_boxes && P.mask_group_boxes && use_side_stream(B, N, ld);
    // masked from-boxes layer, no side stream: K3..K6 of every image and the matrix write as ONE launch (tail_write_kernel), always
    // (up to N = 1024 the score / x sorts could ride in the IoU launch instead, rounds 1-3's iou2d_sort_kernel; replayed as a HIP graph -- the GPU's
    // own time -- this sequence measures the same or better there too: B = 8, N = 128 / 256 / 512 / 1024: 42.4 / 41.0 / 41.5 / 52.1 us
    // against 38.0 / 36.6 / 40.0 / 47.5)
    // (unmasked groups, round 4b: K3..K5's group structure rides in the write launch too, up to N = 4096; the per-group solves and K6 follow)
    if (from_boxes && (P.mask_group_boxes || N <= 4096)) {
        const MatrixWrite mw = {iou_out, ld, !beside};
        return forward_boxes(c, boxes, scores, &mw);
    }
    // every other mode: the matrix by gnms_iou2d's own kernels (the persistent writers for a box set with itself), then the layer.
    // (Rounds 1-3 carried the score sort in the last grid slice of a 64 x 256-tile IoU launch here, iou2d_sort_kernel: 135 us at B = 8,
    // N = 4096 where the writers take 92 and the two sort launches 15; removed in round 4b.)
    int rc;
    if ((rc = gnms_iou2d(boxes, boxes, B, N, N, iou_out, ld, stream))) return rc;
    if (from_boxes) return forward_boxes(c, boxes, scores);
    return forward_matrix(c, scores, iou_out, ld, aligned16(boxes) ? boxes : nullptr);
}

// defined in iou_kernels.hip
int gnms_internal_records_from_params(const float* params, long count, float* rec, hipStream_t st);
int gnms_internal_records_for_layer(const float* params, int B, int N, float* rec, char* ws, const gnms_ws_layout& L, float* xkeys, hipStream_t st);
int gnms_internal_nms_overlap3d(const float* rec, int B, int N, float* out, int64_t ld, hipStream_t st, float thr, int row0 = 0, int row_end = 0x7fffffff);


namespace {
// everything of gnms_forward_with_iou3d that uses the temporary `rec` ([B][N] records, then [B][N] pseudo boxes for the x sort).
// Masked hard-sorted groups: the whole layer runs from the records (threshold bits AND the O(N) single overlaps, same arithmetic
// as the matrix kernel), so nothing waits for the matrix; large images write it on the side stream beside the one-launch tail.
int forward_with_iou3d_on(const LayerCall& c, float* rec, const float* params3d, const float* scores, int64_t ld, float* iou_out) {
    const int B = c.B, N = c.N;
    const gnms_params& P = c.P;
    const gnms_ws_layout& L = c.L;
    hipStream_t st = c.st;
    const bool from_rec = from_records_3d(P);
    int rc;
    if (!from_rec) {
        if ((rc = gnms_internal_records_from_params(params3d, (long)B * N, rec, st))) return rc;
        return gnms_internal_nms_overlap3d(rec, B, N, iou_out, ld, st, P.nms_threshold);
    }
    float* xkeys = rec + (size_t)B * N * gnms_iou3d::kRec;         // [B][N] pseudo boxes; later the rank-ordered records
    if ((rc = gnms_internal_records_for_layer(params3d, B, N, rec, c.ws, L, xkeys, st))) return rc;
    const Write3dRoute route = write3d_route(B, N, ld, iou_out, P.nms_threshold);
    const bool beside = route.beside, chain_in_write = route.in_tail;
    const int sym = (P.nms_threshold >= 0.01f && P.nms_threshold < INFINITY) ? 1 : 0;   // the culled kernel writes full symmetric rows of W
    if (!beside && !chain_in_write && (rc = gnms_internal_nms_overlap3d(rec, B, N, iou_out, ld, st, P.nms_threshold))) return rc;
    // + the cuboids in the column order of the bit-matrix kernel: (z band, x centre).  Bands: so that a slot of 64 consecutive columns is
    // about as deep in z as it is wide in x (a handful of bands of >= 512 cuboids each; one band up to N = 1024)
    // (B = 8 uniform cuboids, bit-matrix kernel: N = 4096 52 / 47 / 46 / 46.5 us with 1 / 4 / 8 / 12 bands, N = 16384 494 / 409 / 407 with 1 / 8 / 15)
    const int bands = std::max(1, std::min(8, N / 512));
    if ((rc = gnms_internal_launch_sorts(c, scores, xkeys, bands))) return rc;
    SideScope scope(st);
    // the part of the write that runs beside the bit-matrix kernel: rows [0, r1) of the all-pairs kernel
    const int r1 = beside ? split_rows(N, 20) : 0;
    if (r1 > 0) {                                                 // first part of the write beside the bit-matrix kernel
        hipStream_t side = nullptr;
        if ((rc = scope.fork(&side, 0))) return rc;
        if ((rc = gnms_internal_nms_overlap3d(rec, B, N, iou_out, ld, side, P.nms_threshold, 0, r1))) return rc;
    }
    if (!sym) {
        // no culling possible below that threshold: the triangular tile set does half the pairs of the square one
        bitmask_rec3d_kernel<<<dim3(gnms_div_up(tri_tile_count(L.NB), 4), 1, B), 256, 0, st>>>(N, c.counts, P.nms_threshold, c.ws, L);
    } else {
        // row groups of 4 blocks where there are plenty of tiles; from N > 4096 the row groups are dealt to the XCDs (see the kernel)
        const long long tiles = (long long)B * L.NB * ((N + 255) / 256);
        const int kbw = tiles >= 32768 ? 4 : 1;                       // (N = 4096: 46 / 48 / 59 us with 1 / 2 / 4; N = 16384: 338 with 2, 325 with 4)
        const int pinned = N > 4096 ? 1 : 0;
        const int nkbg = gnms_div_up(L.NB, kbw), nchunk = (N + 255) / 256;
        const unsigned gx = pinned ? (unsigned)(gnms_div_up(nkbg, 8) * gnms_div_up(nchunk, 4) * 8) : (unsigned)gnms_div_up(nkbg * nchunk, 4);
        if (kbw >= 4)
            bitmask_rec3d_culled_kernel<4><<<dim3(gx, 1, B), 256, 0, st>>>(N, c.counts, P.nms_threshold, c.ws, L, pinned);
        else
            bitmask_rec3d_culled_kernel<1><<<dim3(gx, 1, B), 256, 0, st>>>(N, c.counts, P.nms_threshold, c.ws, L, pinned);
    }
    GNMS_CHECK_LAUNCH();
    if (chain_in_write)                                           // K3..K6 and the matrix in one launch, like the 2D entry
        return gnms_internal_launch_tail_write<kFromRecords>(c, nullptr, rec, iou_out, ld);
    if (beside) {                                                 // see forward_boxes for why the fork sits exactly here
        hipStream_t side = nullptr;
        if ((rc = scope.fork(&side, 1))) return rc;
        if ((rc = gnms_internal_launch_tail<kFromRecords>(c, nullptr, ld, sym, kBesideChainWGs))) return rc;
        if ((rc = gnms_internal_nms_overlap3d(rec, B, N, iou_out, ld, side, P.nms_threshold, r1, N))) return rc;
        return scope.join();
    }
    if (use_tail_kernel(N, sym)) return gnms_internal_launch_tail<kFromRecords>(c, nullptr, ld, sym);
    return launch_separate_tail<kFromRecords>(c, nullptr, ld, sym);
}
}  // namespace

// The 3D analogue of gnms_forward_with_iou2d: cuboid parameters -> the NMS overlap matrix 0.5*(1+GIoU3D) (an output, written by
// iou3d_nms_fast_kernel) -> the layer.  The grouped hard-sort modes take their threshold bits from the records with the same
// instruction sequence that wrote the matrix (bitmask_rec3d_kernel) instead of reading 4 N^2 bytes back; the O(N) overlaps the
// group kernels need are gathered from the matrix.
extern "C" int gnms_forward_with_iou3d(const float* params3d, const float* scores, int B, int N, int64_t ld, const int32_t* counts,
                                       const gnms_params* params, float* iou_out, float* prob, int64_t* order, int64_t* valid,
                                       int64_t* invalid, int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_forward_with_iou3d", &c, B, N, ld, counts, params, workspace, workspace_bytes, stream, false,
                    params3d && scores && iou_out && prob, "gnms_forward_with_iou3d: null pointer", prob, order, valid, invalid, nvalid, ninvalid);
    // records of the whole batch in one stream-ordered temporary (the overlap kernel wants them contiguous); the layer's copy goes
    // into the per-image workspace regions
    float* rec = nullptr;
    GNMS_CHECK_HIP(hipMallocAsync((void**)&rec, (size_t)B * N * (2 * gnms_iou3d::kRec) * sizeof(float), c.st));
    const int rc = forward_with_iou3d_on(c, rec, params3d, scores, ld, iou_out);
    const hipError_t fe = hipFreeAsync(rec, c.st);                // after the side stream, if any, has joined `st`
    if (rc) return rc;
    if (fe != hipSuccess) { gnms_set_error("hipFreeAsync failed: %s", hipGetErrorString(fe)); return GNMS_ERR_HIP; }
    if (!from_records_3d(c.P)) return forward_matrix(c, scores, iou_out, ld);
    return GNMS_OK;
}

extern "C" int gnms_backward(const float* grad_prob, const float* scores, const float* iou, int B, int N, int64_t ld,
                             const int32_t* counts, const gnms_params* params, float* grad_scores, float* grad_iou,
                             void* workspace, size_t workspace_bytes, void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_backward", &c, B, N, ld, counts, params, workspace, workspace_bytes, stream, false,
                    grad_prob && scores && iou && grad_scores, "gnms_backward: null pointer");
    const gnms_params& P = c.P;
    const gnms_ws_layout& L = c.L;
    char* ws = c.ws;
    hipStream_t st = c.st;
    int rc;
    dim3 ge(gnms_div_up(N, 256), B);
    const bool fused_gx = masked_default(P);
    if (!fused_gx) {
        bwd_gx_kernel<<<ge, 256, 0, st>>>(grad_prob, N, counts, P, ws, L);
        GNMS_CHECK_LAUNCH();
    }
    if (grad_iou) GNMS_CHECK_HIP(hipMemsetAsync(grad_iou, 0, sizeof(float) * (size_t)B * N * ld, st));
    if (masked_groups(P)) {
        const int head_blocks = N >= 2048 ? 128 : gnms_div_up(N, 16);
        // GNMS_BWD_PLAN=0: the backward that walks hlist / gstart / glen / gsorted instead of the forward's plan (A/B runs, the bit-for-bit test)
        static const bool by_plan = env_switch("GNMS_BWD_PLAN", 1) != 0;
        if (fused_gx && by_plan) {
            bwd_plan_kernel<<<ge, 256, 0, st>>>(grad_prob, N, ws, L, grad_scores, grad_iou ? 1 : 0);
            GNMS_CHECK_LAUNCH();
        } else if (fused_gx) {
            bwd_masked_fused_kernel<<<dim3(ge.x + head_blocks, B), 256, 0, st>>>(grad_prob, N, counts, P, ws, L, grad_scores, (int)ge.x);
            GNMS_CHECK_LAUNCH();
        } else {
            bwd_masked_kernel<<<ge, 256, 0, st>>>(N, counts, P, ws, L, grad_scores);
            GNMS_CHECK_LAUNCH();
            bwd_masked_heads_kernel<<<dim3(head_blocks, B), 256, 0, st>>>(N, P, ws, L, grad_scores);
            GNMS_CHECK_LAUNCH();
        }
        if (grad_iou) {
            bwd_masked_iou_kernel<<<ge, 256, 0, st>>>(iou, N, (long)ld, counts, P, ws, L, grad_iou);
            GNMS_CHECK_LAUNCH();
        }
    } else if (P.group_boxes) {
        return launch_solve_groups<kBackward, kFromMatrix>(c, iou, ld, grad_scores, grad_iou);
    } else {
        const float* Ps = reinterpret_cast<const float*>(ws + (size_t)B * L.per_image);   // written by the forward pass
        ungrouped_backward_prepare_kernel<<<dim3(gnms_div_up(N, 1024), B), 1024, 0, st>>>(N, ws, L);
        GNMS_CHECK_LAUNCH();
        if ((rc = allow_lds(ungrouped_solve_backward_kernel, kUngroupedBwdLds))) return rc;
        ungrouped_solve_backward_kernel<<<dim3(gnms_div_up(N, kUB), B), kUThreads, kUngroupedBwdLds, st>>>(N, counts, P, ws, L, Ps, grad_scores);
        GNMS_CHECK_LAUNCH();
        if (grad_iou) {
            ungrouped_grad_iou_kernel<<<dim3(gnms_div_up(N, 256), N, B), 256, 0, st>>>(iou, N, (long)ld, counts, P, ws, L, grad_iou);
            GNMS_CHECK_LAUNCH();
        }
    }
    return GNMS_OK;
}

// ------------------------------------------------------------------------------------------------
// from-boxes path: same layer, the N x N matrix never materialised (grouped modes)
// ------------------------------------------------------------------------------------------------
namespace {
int forward_boxes(const LayerCall& c, const float* boxes, const float* scores, const MatrixWrite* mw) {
    const int B = c.B, N = c.N;
    const gnms_params& P = c.P;
    hipStream_t st = c.st;
    int rc;
    // Large images: the matrix write is ONE persistent launch (write_staged_kernel) on the side stream that leaves B CUs without a
    // writer workgroup; forked behind the bit-matrix kernel, so that what runs beside it on the caller's stream is the one-workgroup-
    // per-image tail, which finds those CUs free (B = 8, N = 16384: write 1.60 ms = 5.4 TB/s, the tail 1.03 ms beside it, step 2.04 ms;
    // with gnms_iou2d's kernel in two launches beside bit matrix and tail: 2.13).  Forked in front of the bit-matrix kernel the two
    // VALU-heavy kernels share the SIMDs and the sum stays the same (write 1.97 ms, step 2.01); forked in front of the sorts as well,
    // those crawl (step 2.35).
    const bool persistent_write = mw && !mw->one_launch && (mw->ld % 4 == 0) && ((uintptr_t)mw->out % 16 == 0) && (N % 4 == 0);
    if (mw && mw->one_launch) {                                   // a small image: sort, table, chain and the matrix write as ONE launch
        bool launched = false;
        if ((rc = launch_one_boxes(c, scores, boxes, mw->out, mw->ld, &launched)) || launched) return rc;
    }
    if ((rc = gnms_internal_launch_sorts(c, scores, boxes))) return rc;
    if (persistent_write) {
        SideScope whole(st);
        hipStream_t side = nullptr;
        if ((rc = gnms_internal_launch_bitmask_boxes(c, boxes))) return rc;
        if ((rc = whole.fork(&side, 0))) return rc;
        // (the scan on at most kBesideChainWGs workgroups per image: their CUs are the ones the persistent write leaves free)
        if ((rc = gnms_internal_launch_tail<kFromBoxes>(c, boxes, N, 1, kBesideChainWGs))) return rc;
        if ((rc = launch_write_staged(boxes, boxes, B, N, N, mw->out, mw->ld, B * leaders_chain_wgs(N, 1, kBesideChainWGs), side))) return rc;
        return whole.join();
    }
    if (mw && mw->one_launch) {
        if ((rc = gnms_internal_launch_bitmask_boxes(c, boxes))) return rc;
        if ((rc = gnms_internal_launch_tail_write<kFromBoxes>(c, boxes, boxes, mw->out, mw->ld))) return rc;
        if (P.mask_group_boxes) return GNMS_OK;
        // unmasked groups: the chain stopped behind K5's group structure
        if ((rc = launch_solve_groups<kForward, kFromBoxes>(c, boxes, N, nullptr, nullptr))) return rc;
        return launch_finalize(c);
    }
    SideScope beside(st);
    const int r1 = mw ? split_rows(N, 20) : 0;
    if (r1 > 0) {                        // first part of the write beside the bit-matrix kernel (small workgroups: they interleave)
        hipStream_t side = nullptr;
        if ((rc = beside.fork(&side, 0))) return rc;
        if ((rc = gnms_internal_iou2d_rows(boxes, B, N, mw->out, mw->ld, side, 0, r1))) return rc;
    }
    if ((rc = gnms_internal_launch_bitmask_boxes(c, boxes))) return rc;
    if (mw) {
        // Large images: the rest of the layer is one workgroup per image (K3..K6 in one launch) and the matrix write runs beside
        // it on the side stream.  The write is forked HERE and not earlier because its workgroups take every free wave slot: a
        // 16-wave, 128-KiB-LDS workgroup that becomes ready while the write runs is not placed before the write drains (measured:
        // sort_merge_kernel waited 1.85 ms).  Forked here, the tail's B workgroups are resident before the side stream has seen
        // the event (same-queue successor ~2 us, cross-queue event ~25 us), and then keep their CUs until the layer is done.
        hipStream_t side = nullptr;
        if ((rc = beside.fork(&side, 1))) return rc;
        if ((rc = gnms_internal_launch_tail<kFromBoxes>(c, boxes, N, 1, kBesideChainWGs))) return rc;
        if ((rc = gnms_internal_iou2d_rows(boxes, B, N, mw->out, mw->ld, side, r1, N))) return rc;
        return beside.join();
    }
    // (sym 1: bitmask_boxes_kernel wrote full symmetric rows)
    if (P.mask_group_boxes && use_tail_kernel(N, 1)) return gnms_internal_launch_tail<kFromBoxes>(c, boxes, N, 1);
    return launch_separate_tail<kFromBoxes>(c, boxes, N, 1);
}
}  // namespace

extern "C" int gnms_forward_from_boxes(const float* boxes, const float* scores, int B, int N, const int32_t* counts,
                                       const gnms_params* params, float* prob, int64_t* order, int64_t* valid, int64_t* invalid,
                                       int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes, void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_forward_from_boxes", &c, B, N, N, counts, params, workspace, workspace_bytes, stream, true, boxes && scores && prob,
                    "gnms_forward_from_boxes: null boxes/scores/prob", prob, order, valid, invalid, nvalid, ninvalid);
    GNMS_CHECK_ARG(aligned16(boxes), "gnms_forward_from_boxes: boxes must be 16-byte aligned");
    return forward_boxes(c, boxes, scores);
}

extern "C" int gnms_backward_from_boxes(const float* grad_prob, const float* boxes, const float* scores, int B, int N,
                                        const int32_t* counts, const gnms_params* params, float* grad_scores, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    LayerCall c;
    GNMS_BEGIN_CALL("gnms_backward_from_boxes", &c, B, N, N, counts, params, workspace, workspace_bytes, stream, true,
                    grad_prob && boxes && scores && grad_scores, "gnms_backward_from_boxes: null pointer");
    if (c.P.mask_group_boxes)          // the masked backward never touches the overlaps
        return gnms_backward(grad_prob, scores, boxes, B, N, N, counts, params, grad_scores, nullptr, workspace, workspace_bytes, stream);
    bwd_gx_kernel<<<dim3(gnms_div_up(N, 256), B), 256, 0, c.st>>>(grad_prob, N, counts, c.P, c.ws, c.L);
    GNMS_CHECK_LAUNCH();
    return launch_solve_groups<kBackward, kFromBoxes>(c, boxes, N, grad_scores, nullptr);
}

// ------------------------------------------------------------------------------------------------
// backward with the gradient w.r.t. the geometry: the 2D boxes of gnms_forward_with_iou2d, the cuboids of
// gnms_forward_with_iou3d.  One body, backward_geometry<G>; G adds to the masked kernel's geometry what the dense route calls.
// ------------------------------------------------------------------------------------------------
namespace {
struct BoxesBackward : MaskedBoxes {
    static constexpr bool kAlign16 = true;                           // the kernels load a box, and store its gradient, as one float4
    static int write_matrix(const float* boxes, int B, int N, const gnms_params&, float* m, int64_t ld, void* stream) {
        return gnms_iou2d(boxes, boxes, B, N, N, m, ld, stream);
    }
    static size_t pair_workspace_bytes(int B, int N) { return gnms_iou2d_backward_workspace_bytes(B, N, N); }
    static int pair_backward(const float* boxes, const float* grad_iou, int B, int N, int64_t ld, float* grad_boxes, void* ws, size_t bytes, void* stream) {
        return gnms_iou2d_backward(boxes, nullptr, grad_iou, B, N, N, ld, grad_boxes, nullptr, ws, bytes, stream);
    }
};
struct CuboidsBackward : MaskedCuboids {
    static constexpr bool kAlign16 = false;
    static int write_matrix(const float* params3d, int B, int N, const gnms_params& P, float* m, int64_t ld, void* stream) {
        return gnms_nms_overlap3d_from_params(params3d, B, N, P.nms_threshold, m, ld, stream);    // the forward's own writer, at its threshold
    }
    static size_t pair_workspace_bytes(int B, int N) { return gnms_iou3d_backward_workspace_bytes(B, N, N); }
    static int pair_backward(const float* params3d, const float* grad_iou, int B, int N, int64_t ld, float* grad_params3d, void* ws, size_t bytes,
                             void* stream) {
        return gnms_iou3d_backward(params3d, nullptr, grad_iou, B, N, N, ld, 2, grad_params3d, nullptr, ws, bytes, stream);
    }
};

// the dense route's scratch: the matrix gradient | the matrix, where the caller kept none | the pair backward's workspace
struct GeometryScratch { size_t grad_iou, iou, reduce, total; };
template <class G>
GeometryScratch geometry_scratch(int B, int N, int64_t ld, bool have_matrix) {
    GeometryScratch s;
    s.grad_iou = gnms_align_up(sizeof(float) * (size_t)B * N * ld, 256);
    s.iou = have_matrix ? 0 : s.grad_iou;
    s.reduce = G::pair_workspace_bytes(B, N);
    s.total = s.grad_iou + s.iou + s.reduce;
    return s;
}
template <class G>
size_t geometry_scratch_bytes(int B, int N, int64_t ld, const gnms_params* params, int have_matrix, int route) {
    if (!params || B <= 0 || N <= 0 || ld < N || boxes_sparse_route(*params, route)) return 0;
    return geometry_scratch<G>(B, N, ld, have_matrix != 0).total;
}

template <class G>
int backward_geometry(const char* name, const float* grad_prob, const float* rows, const float* scores, int B, int N, const int32_t* counts,
                      const gnms_params* params, float* grad_scores, float* grad_rows, const float* matrix, int64_t ld, int route, void* scratch,
                      size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    LayerCall c;
    char null_msg[64];
    snprintf(null_msg, sizeof(null_msg), "%s: null pointer", name);
    GNMS_CHECK_ARG(route == GNMS_BOXES_ROUTE_AUTO || route == GNMS_BOXES_ROUTE_DENSE, "%s: unknown route %d", name, route);
    GNMS_BEGIN_CALL(name, &c, B, N, ld, counts, params, workspace, workspace_bytes, stream, false,
                    grad_prob && rows && scores && grad_scores && grad_rows, null_msg);
    if (G::kAlign16) GNMS_CHECK_ARG(aligned16(rows) && aligned16(grad_rows), "%s: boxes and grad_boxes must be 16-byte aligned", name);
    int rc;
    if (boxes_sparse_route(c.P, route)) {
        // (the masked backward never dereferences the matrix pointer when no matrix gradient is asked for)
        if ((rc = gnms_backward(grad_prob, scores, rows, B, N, N, counts, params, grad_scores, nullptr, workspace, workspace_bytes, stream))) return rc;
        const int elem_blocks = gnms_div_up(N, 256), head_blocks = N >= 2048 ? 128 : gnms_div_up(N, 16);
        bwd_masked_geometry_kernel<G><<<dim3(elem_blocks + head_blocks, B), 256, 0, c.st>>>(grad_prob, rows, N, counts, c.P, c.ws, c.L, grad_rows,
                                                                                            elem_blocks);
        GNMS_CHECK_LAUNCH();
        return GNMS_OK;
    }
    // every other mode: the layer's matrix gradient into the scratch matrix, then the pair backward with the geometry on both sides
    const GeometryScratch s = geometry_scratch<G>(B, N, ld, matrix != nullptr);
    GNMS_CHECK_ARG(scratch != nullptr && (uintptr_t)scratch % 256 == 0, "%s: scratch is NULL or not 256-byte aligned", name);
    if (scratch_bytes < s.total) {
        gnms_set_error("%s: scratch too small (%zu < %zu)", name, scratch_bytes, s.total);
        return GNMS_ERR_WORKSPACE;
    }
    float* grad_iou = static_cast<float*>(scratch);
    if (!matrix) {
        float* m = reinterpret_cast<float*>(static_cast<char*>(scratch) + s.grad_iou);
        if ((rc = G::write_matrix(rows, B, N, c.P, m, ld, stream))) return rc;
        matrix = m;
    }
    if ((rc = gnms_backward(grad_prob, scores, matrix, B, N, ld, counts, params, grad_scores, grad_iou, workspace, workspace_bytes, stream))) return rc;
    return G::pair_backward(rows, grad_iou, B, N, ld, grad_rows, static_cast<char*>(scratch) + s.grad_iou + s.iou, s.reduce, stream);
}
}  // namespace

extern "C" size_t gnms_backward_boxes_scratch_bytes(int B, int N, int64_t ld, const gnms_params* params, int have_iou, int route) {
    return geometry_scratch_bytes<BoxesBackward>(B, N, ld, params, have_iou, route);
}

extern "C" int gnms_backward_boxes(const float* grad_prob, const float* boxes, const float* scores, int B, int N, const int32_t* counts,
                                   const gnms_params* params, float* grad_scores, float* grad_boxes, const float* iou, int64_t ld, int route,
                                   void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return backward_geometry<BoxesBackward>("gnms_backward_boxes", grad_prob, boxes, scores, B, N, counts, params, grad_scores, grad_boxes, iou, ld, route,
                                            scratch, scratch_bytes, workspace, workspace_bytes, stream);
}

// host code only (the table stands in include/groomed_nms_hip.h); the same gate as gnms_backward_cuboids branches on
extern "C" int gnms_backward_cuboids_reads(const gnms_params* params, const void* params3d, int route) {
    GNMS_CHECK_ARG(params != nullptr, "gnms_backward_cuboids_reads: params is NULL");
    GNMS_CHECK_ARG(params3d != nullptr, "gnms_backward_cuboids_reads: params3d is NULL");
    GNMS_CHECK_ARG(route == GNMS_BOXES_ROUTE_AUTO || route == GNMS_BOXES_ROUTE_DENSE, "gnms_backward_cuboids_reads: unknown route %d", route);
    return GNMS_BWD_READS_BOXES | (boxes_sparse_route(*params, route) ? 0 : GNMS_BWD_READS_MATRIX);
}

extern "C" size_t gnms_backward_cuboids_scratch_bytes(int B, int N, int64_t ld, const gnms_params* params, int have_overlap, int route) {
    return geometry_scratch_bytes<CuboidsBackward>(B, N, ld, params, have_overlap, route);
}

extern "C" int gnms_backward_cuboids(const float* grad_prob, const float* params3d, const float* scores, int B, int N, const int32_t* counts,
                                     const gnms_params* params, float* grad_scores, float* grad_params3d, const float* overlap, int64_t ld,
                                     int route, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return backward_geometry<CuboidsBackward>("gnms_backward_cuboids", grad_prob, params3d, scores, B, N, counts, params, grad_scores, grad_params3d,
                                              overlap, ld, route, scratch, scratch_bytes, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// get_groups as a stand-alone entry (lib/groomed_nms.py:208-270)
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void export_groups_kernel(int N, char* ws, gnms_ws_layout L, int* __restrict__ group_of, int* __restrict__ pos_in_group,
                                     int* __restrict__ ngroups) {
    // group id = index of the group's leader among the leaders in creation order, minus the empty groups before it
    using namespace gnms;
    ImgPtrs I = img_ptrs(ws, L, 0);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *ngroups = I.misc[0];
    if (k >= N) return;
    const int c = I.order[k];
    const int h = I.head[k];
    int gid = -1;
    if (h >= 0) {
        const int lr = I.rem[k];                              // the group's leader
        gid = I.leadpfx[lr >> 6] + __builtin_popcountll(I.leadw[lr >> 6] & ((1ull << (lr & 63)) - 1ull));
    }
    group_of[c] = gid;
    pos_in_group[c] = I.gpos[k];
}
}  // namespace

extern "C" int gnms_get_groups(const float* scores, const float* iou, int N, int64_t ld, float group_threshold, int group_size,
                               int32_t* group_of, int32_t* pos_in_group, int32_t* ngroups_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    gnms_params P;
    gnms_default_params(&P);
    P.nms_threshold = group_threshold;
    P.group_size = group_size;
    P.mask_group_boxes = 0;   // grouping only: skip the fused rescoring
    int rc = check_common("gnms_get_groups", 1, N, ld, &P, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    GNMS_CHECK_ARG(ngroups_out != nullptr, "gnms_get_groups: ngroups_out is NULL");
    if (N == 0) { GNMS_CHECK_HIP(hipMemsetAsync(ngroups_out, 0, sizeof(int32_t), st)); return GNMS_OK; }
    GNMS_CHECK_ARG(scores && iou && group_of && pos_in_group, "gnms_get_groups: null pointer");
    const LayerCall c = make_call(1, N, nullptr, P, workspace, stream);
    GNMS_DISPATCH_SORT(c.P2, {
        if ((rc = allow_lds(sort_scores_kernel<E>, c.sort_lds()))) return rc;
        sort_scores_kernel<E><<<1, c.sort_threads(), c.sort_lds(), st>>>(scores, N, nullptr, c.ws, c.L, c.P2, nullptr, nullptr, 0);
    });
    GNMS_CHECK_LAUNCH();
    // grouping pipeline K2..K5, as the unmasked layer runs it
    const int sym = matrix_sym_detection(N) ? 2 : 0;
    if ((rc = gnms_internal_launch_bitmask(c, iou, ld, sym ? 1 : 0))) return rc;
    if ((rc = launch_leaders_attribute<kFromMatrix>(c, iou, ld, sym))) return rc;
    if ((rc = launch_groups<kFromMatrix>(c, iou, ld))) return rc;
    export_groups_kernel<<<gnms_div_up(N, 256), 256, 0, st>>>(N, c.ws, c.L, group_of, pos_in_group, ngroups_out);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

// ------------------------------------------------------------------------------------------------
// pruning_function, elementwise (lib/groomed_nms.py:167-189)
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void prune_kernel(const float* __restrict__ x, long long count, float thr, float temp, int method, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x)
        out[i] = gnms_prune(x[i], thr, temp, method);
}
}  // namespace

namespace {
__global__ void prune_grad_kernel(const float* __restrict__ x, const float* __restrict__ g, long long count, float thr, float temp, int method,
                                  float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x)
        out[i] = g[i] * gnms_prune_grad(x[i], thr, temp, method);
}
}  // namespace

extern "C" int gnms_pruning_function_backward(const float* iou, const float* grad_out, int64_t count, float nms_threshold, float temperature,
                                              int pruning_method, float* grad_iou, void* stream) {
    if (pruning_method < 0 || pruning_method > 2) {
        gnms_set_error("gnms_pruning_function_backward: Pruning method not implemented! (pruning_method=%d)", pruning_method);
        return GNMS_ERR_UNSUPPORTED;
    }
    GNMS_CHECK_ARG(count >= 0, "gnms_pruning_function_backward: negative count");
    if (count == 0) return GNMS_OK;
    GNMS_CHECK_ARG(iou && grad_out && grad_iou, "gnms_pruning_function_backward: null pointer");
    long long blocks = (count + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    prune_grad_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(iou, grad_out, (long long)count, nms_threshold, temperature,
                                                                         pruning_method, grad_iou);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_pruning_function(const float* iou, int64_t count, float nms_threshold, float temperature, int pruning_method,
                                     float* out, void* stream) {
    if (pruning_method < 0 || pruning_method > 2) {
        gnms_set_error("gnms_pruning_function: Pruning method not implemented! (pruning_method=%d)", pruning_method);
        return GNMS_ERR_UNSUPPORTED;
    }
    GNMS_CHECK_ARG(count >= 0, "gnms_pruning_function: negative count");
    if (count == 0) return GNMS_OK;
    GNMS_CHECK_ARG(iou && out, "gnms_pruning_function: null pointer");
    long long blocks = (count + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    prune_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(iou, (long long)count, nms_threshold, temperature, pruning_method, out);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
