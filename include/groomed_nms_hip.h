/*
 * groomed_nms_hip.h -- C ABI of libgroomed_nms_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the GrooMeD-NMS hot path of abhi1kumar/groomed_nms.  Citations are
 * file:line in the reference checkout.  The reference's boundary for this path is a Python call
 * (lib/groomed_nms.py:10 differentiable_nms, imported at lib/loss/rpn_3d.py:14 and
 * lib/rpn_util.py:18) plus ONE true C symbol, `_nms` (lib/nms/gpu_nms.hpp:1-2, bound by Cython at
 * lib/nms/gpu_nms.pyx:13-14).  `_nms` is exported here with the identical signature; the gnms_*
 * functions are what a ctypes/Cython/cffi binding of lib/groomed_nms.py and of the overlap helpers
 * in lib/core.py binds (see INTEGRATION.md for the stubs).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host;
 *   - calls are asynchronous and ordered on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream); no hidden synchronisation and no hidden allocation, except `_nms`, which keeps
 *     the reference's blocking host-pointer contract, and the 3D entries (gnms_iou3d_*, gnms_forward_with_iou3d),
 *     which take a stream-ordered temporary (hipMallocAsync/hipFreeAsync) of 48-64 bytes per box for the cuboid records;
 *     and gnms_iou2d of a box set with itself (boxes_a == boxes_b, N <= 4096), whose FIRST call on a device allocates a 1-MiB ring
 *     of claim counters that lives as long as the process (hipMalloc: make that first call outside stream capture; later calls
 *     allocate nothing and are capturable);
 *   - gnms_forward_with_iou2d / _iou3d on images of more than 4096 boxes issue the matrix write on a library-owned stream
 *     (one per device, lowest priority) that forks from `stream` and joins it again before the call returns control of the
 *     ordering to the caller: to the caller everything is still ordered on `stream` (earlier work happens before, later work
 *     after), also under stream capture (the fork/join is captured as a branch of the graph);
 *   - a batch is B images of up to N boxes; image b uses the first counts[b] boxes (counts may be
 *     NULL: every image has N).  Scores are [B][N]; overlap matrices are [B][N][ld] row-major with
 *     row stride ld >= N elements (image stride N*ld);
 *   - return value: 0 on success, negative gnms_status on failure; gnms_last_error() gives the
 *     message of the calling thread's last failure (the reference prints CUDA errors and carries
 *     on, lib/nms/nms_kernel.cu:12-19; this library never does that).
 *   - fp32 arithmetic without FMA contraction, IEEE division: results are bit-identical to the
 *     CPU restatement in oracle/ wherever that one is fp32-sequential (overlaps, default rescoring).
 */
#ifndef GROOMED_NMS_HIP_H
#define GROOMED_NMS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNMS_ABI_VERSION 1
#define GNMS_MAX_BOXES 16384 /* per image; the in-LDS sorts and merges hold 16384 64-bit keys in 128 KiB of the CU's 160 KiB */

typedef enum gnms_status {
    GNMS_OK = 0,
    GNMS_ERR_INVALID_ARGUMENT = -1,
    GNMS_ERR_UNSUPPORTED = -2, /* e.g. N > GNMS_MAX_BOXES, unknown pruning method (reference: NotImplementedError) */
    GNMS_ERR_HIP = -3,
    GNMS_ERR_WORKSPACE = -4
} gnms_status;

/* lib/groomed_nms.py:167-189 pruning_function */
typedef enum gnms_pruning { GNMS_PRUNE_LINEAR = 0, GNMS_PRUNE_SIGMOIDAL = 1, GNMS_PRUNE_SOFT_NMS = 2 } gnms_pruning;

/* keyword arguments of differentiable_nms (lib/groomed_nms.py:10), same names, same defaults */
typedef struct gnms_params {
    float nms_threshold;            /* 0.4  */
    float temperature;              /* 0.01 (unused by "linear") */
    float valid_box_prob_threshold; /* 0.3  */
    int32_t pruning_method;         /* gnms_pruning */
    int32_t return_sorted_prob;     /* 0 */
    int32_t group_boxes;            /* 1 */
    int32_t mask_group_boxes;       /* 1 */
    int32_t group_size;             /* 100 */
    int32_t presorted;              /* 0.  1 = the soft-sort hand-off (lib/groomed_nms.py:42-45): scores/iou are
                                       consumed in INPUT order (prune matrix, rescoring, returned probabilities), only
                                       the grouping re-sorts by score as get_groups does (:213-214). */
} gnms_params;

void gnms_default_params(gnms_params* p);
int gnms_abi_version(void);
const char* gnms_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Pairwise overlaps (lib/core.py)
 * ------------------------------------------------------------------------------------------- */

/* iou(box_a, box_b, mode='combinations')  lib/core.py:480-508 (+ intersect :178-218).
 * boxes_a [B][M][4], boxes_b [B][N][4] as (x1,y1,x2,y2); out[b][i][j] = IoU(a_i, b_j), row stride ld >= N.
 * No +1 pixel; a zero-area pair yields 0/0 = NaN exactly like the reference. */
int gnms_iou2d(const float* boxes_a, const float* boxes_b, int B, int M, int N, float* out, int64_t ld, void* stream);

/* backward of gnms_iou2d: the cotangent grad [B][M][ld] of the matrix contracted with dIoU/dbox (torch autograd's conventions for
 * lib/core.py:499-508: a tied max / min splits its gradient evenly, the clamp passes it at 0).
 *   d_boxes_a [B][M][4] = sum_j grad[i][j] dIoU(a_i, b_j)/da_i,  d_boxes_b [B][N][4] = sum_i grad[i][j] dIoU(a_i, b_j)/db_j.
 * Either output may be NULL (not both).  boxes_b == NULL means boxes_a on both sides (M == N): both roles are summed into d_boxes_a,
 * d_boxes_b must be NULL.  Every element of a given output is written.  A pair whose cotangent is exactly 0 contributes nothing
 * (torch: 0 * NaN for a zero-area pair); everything else is plain IEEE fp32.  grad is read once; the sums go through per-tile partial
 * slabs in `workspace` (gnms_iou2d_backward_workspace_bytes(B, M, N) bytes, 256-byte aligned) added in a fixed order: no float
 * atomics, the same inputs give the same bits.  Stream-ordered, no allocation, graph-capturable. */
size_t gnms_iou2d_backward_workspace_bytes(int B, int M, int N);
int gnms_iou2d_backward(const float* boxes_a, const float* boxes_b, const float* grad, int B, int M, int N, int64_t ld, float* d_boxes_a,
                        float* d_boxes_b, void* workspace, size_t workspace_bytes, void* stream);

/* backward of gnms_iou3d_from_params (method 0, 1, 2) and of gnms_nms_overlap3d_from_params (method 2: its two expressions share one
 * analytic derivative): the cotangent grad [B][M][ld] of the matrix contracted with d overlap / d cuboid, through the corner AABBs of
 * get_corners_of_cuboid.
 *   d_params_a [B][M][7] = sum_j grad[i][j] d f(a_i, b_j)/d a_i,  d_params_b [B][N][7] = sum_i grad[i][j] d f(a_i, b_j)/d b_j,
 *   each row (x3d, y3d, z3d, w3d, h3d, l3d, ry3d).
 * torch autograd's conventions for lib/core.py:305-421: a tied elementwise max / min of the two boxes' edges splits evenly; the x and z
 * intersection extents pass the gradient at 0 (clamp), the y intersection extent and the three hull extents give 1/2 at exactly 0
 * (torch.max(zeros, .)).  One deliberate difference: where a box's own corners tie (sin ry or cos ry exactly 0: ry = +-0 in float32)
 * they share the gradient (sgn 0 = 0), so d ry is the symmetric value there; the reference sends it all to one unspecified corner.
 * Ties and clamps are decided on the float32 extents the forward saw.  Either output may be NULL (not both).  params_b == NULL means
 * params_a on both sides (M == N): both roles are summed into d_params_a, d_params_b must be NULL.  Every element of a given output is
 * written.  A pair whose cotangent is exactly 0 contributes nothing; everything else is plain IEEE fp32.  grad is read once; the sums go
 * through per-tile partial slabs in `workspace` (gnms_iou3d_backward_workspace_bytes(B, M, N) bytes, 256-byte aligned; it also holds
 * the boxes' records) added in a fixed order: no float atomics, the same inputs give the same bits.  No alignment is asked of the
 * parameters or the outputs (28-byte rows).  Stream-ordered, no allocation, graph-capturable. */
size_t gnms_iou3d_backward_workspace_bytes(int B, int M, int N);
int gnms_iou3d_backward(const float* params_a, const float* params_b, const float* grad, int B, int M, int N, int64_t ld, int method,
                        float* d_params_a, float* d_params_b, void* workspace, size_t workspace_bytes, void* stream);

/* get_corners_of_cuboid  lib/math_3d.py:364-435 (torch branch, iou_3d_convention=True).
 * params [count][7] = (x3d, y3d, z3d, w3d, h3d, l3d, ry3d) -> corners [count][3][8]. */
int gnms_corners_of_cuboid(const float* params, int64_t count, float* corners, void* stream);

/* The float64 NumPy branches of the same two helpers -- what the reference's inference call site runs (lib/rpn_util.py:1292-1320:
 * `aboxes` is float64 after the hstack at :1258): lib/core.py:205-207, 512-513 (iou in float64, rounded to fp32 once by
 * lib/groomed_nms.py:36) and lib/math_3d.py:438-490 (corners in float64 before `.float()`).  Same layouts as above with double
 * elements; the IoU matrix is bit-identical to NumPy's IEEE double arithmetic.  trig_f32 != 0: cos / sin of the yaw in fp32, widened
 * (np.cos on a float32 `ry3d`, the dtype that call site passes). */
int gnms_iou2d_f64(const double* boxes_a, const double* boxes_b, int B, int M, int N, double* out, int64_t ld, void* stream);
int gnms_corners_of_cuboid_f64(const double* params, int64_t count, int trig_f32, double* corners, void* stream);

/* iou3d_approximate(corners_b1, corners_b2, mode="combinations", method=...)  lib/core.py:305-421.
 * corners_a [B][M][3][8], corners_b [B][N][3][8].  Inputs are const (the reference overwrites them, :379-380).
 *   method 0 "normal", 1 "generalized", 2 = 0.5*(1+generalized): what both callers feed the NMS
 *   (lib/loss/rpn_3d.py:781, lib/rpn_util.py:1312).
 * iou_bev may be NULL.  Outputs [B][M][ld]. */
int gnms_iou3d_approximate(const float* corners_a, const float* corners_b, int B, int M, int N, int method,
                           float* iou_bev, float* iou_3d, int64_t ld, void* stream);

/* same, with get_corners_of_cuboid fused as the prologue: params_a [B][M][7], params_b [B][N][7] */
int gnms_iou3d_from_params(const float* params_a, const float* params_b, int B, int M, int N, int method,
                           float* iou_bev, float* iou_3d, int64_t ld, void* stream);

/* iou3d(corners_b1, corners_b2, vol)  lib/core.py:246-302: the EXACT IoU of two rotated cuboids (the reference intersects the
 * bird's-eye-view footprints with shapely).  Footprint = the quadrilateral of corners 7, 2, 3, 6 in (x, z) (:289-294); y overlap
 * = max(0, min(ymax) - max(ymin)) over all 8 corners (:282-286);
 *   iou_bev = I / (area_a + area_b - I),   iou_3d = I * y_overlap / (vol - I * y_overlap)   (:296-300).
 * Geometry in float64 (as GEOS), no clamping: 0/0 yields NaN like the reference (two zero-area footprints).  Footprints must be
 * convex quadrilaterals, of either orientation (both corner conventions of the reference give one); non-convex or
 * self-intersecting quadrilaterals are NOT supported.
 * corners_a [B][M][3][8], corners_b [B][N][3][8] -> iou_bev, iou_3d [B][M][ld] fp32, ld >= N.  Either output may be NULL, not both.
 *   volume_mode 0: vol = sum of the boxes' own volumes (|footprint area| * y extent);
 *               1: vol = sum of the corner AABB volumes, get_volume (:452-456) -- what iou3d uses when vol is None (:276-277).
 * No allocation: capturable in a graph. */
int gnms_iou3d_exact(const float* corners_a, const float* corners_b, int B, int M, int N, int volume_mode,
                     float* iou_bev, float* iou_3d, int64_t ld, void* stream);

/* same, with get_corners_of_cuboid fused as the prologue (the arithmetic of gnms_corners_of_cuboid, hence bit-identical to
 * gnms_corners_of_cuboid followed by gnms_iou3d_exact): params_a [B][M][7], params_b [B][N][7] = (x, y, z, w, h, l, ry) */
int gnms_iou3d_exact_from_params(const float* params_a, const float* params_b, int B, int M, int N, int volume_mode,
                                 float* iou_bev, float* iou_3d, int64_t ld, void* stream);

/* The drop-in's form: `count` pairs (corners_a[i], corners_b[i]), float64 corners [count][3][8] each.  vol: per-pair sums of the
 * two volumes [count] as the reference's `vol` argument, or NULL = the corner AABB volumes (:276-277).  iou_bev / iou_3d [count]
 * float64, either may be NULL, not both. */
int gnms_iou3d_exact_list_f64(const double* corners_a, const double* corners_b, int64_t count, const double* vol,
                              double* iou_bev, double* iou_3d, void* stream);

/* The matrix both reference callers hand to the NMS in 3D mode: 0.5 * (1 + GIoU3D) of the cuboids' corner AABBs
 * (lib/loss/rpn_3d.py:778-781, lib/rpn_util.py:1309-1312), params3d [B][N][7] -> out [B][N][ld], when the caller knows the
 * threshold the layer will apply.  Same values as gnms_iou3d_from_params(method 2) to within 2e-6, but HBM-write bound instead of
 * division bound: one reciprocal per pair (0.5 * (i3 vh + u3^2) / (u3 vh)), and every entry within 8e-6 of `nms_threshold` is
 * replaced by the reference's exact operation order, so that `entry > nms_threshold` takes the reference's decision for every
 * pair.  gnms_forward_with_iou3d writes its matrix with the same kernel. */
int gnms_nms_overlap3d_from_params(const float* params3d, int B, int N, float nms_threshold, float* out, int64_t ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GrooMeD-NMS layer (lib/groomed_nms.py:10-129), hard sort.  Soft sort = gnms_soft_sort + presorted=1.
 * ------------------------------------------------------------------------------------------- */

/* bytes of the workspace gnms_forward needs for (B, N) with these params (NULL: the defaults).  The same buffer carries the
 * state that gnms_backward reads, so keep it alive and untouched between the two calls.  Grouped modes: ~30 N-sized arrays +
 * the N^2/8-byte bit matrix per image; ungrouped mode (group_boxes = 0) adds a 4 N^2-byte scratch matrix per image (the
 * sorted strictly-lower-triangular copy the reference also makes, lib/groomed_nms.py:48). */
size_t gnms_workspace_bytes(int B, int N, const gnms_params* params);

/* forward.  scores [B][N], iou [B][N][ld].
 *   prob    [B][N]  third return value (:124-129): rescored probabilities in descending-input-score
 *                   order (grouped: un-thresholded clone; ungrouped: thresholded; return_sorted_prob:
 *                   thresholded and sorted).  presorted=1: input order.
 *   order   [B][N]  rank -> input index (the `indices` of :41), int64
 *   valid   [B][N]  first return value, first nvalid[b] entries (input indices, by descending rescored prob)
 *   invalid [B][N]  second return value, first ninvalid[b] entries
 *   nvalid, ninvalid [B] int32 (NaN probabilities are in neither list, :118-123)
 * order/valid/invalid/nvalid/ninvalid may each be NULL if not wanted. */
int gnms_forward(const float* scores, const float* iou, int B, int N, int64_t ld, const int32_t* counts,
                 const gnms_params* params, float* prob, int64_t* order, int64_t* valid, int64_t* invalid,
                 int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes, void* stream);

/* gnms_iou2d + gnms_forward in one call, as lib/loss/rpn_3d.py:772-791 runs them back to back: boxes [B][N][4] ->
 * iou_out [B][N][ld] (kept for the caller) -> the outputs of gnms_forward.  With the boxes at hand the grouped hard-sort
 * modes take their threshold bits and group overlaps from the boxes (the from-boxes kernels below, bit-identical) instead
 * of reading back the matrix they just wrote: nothing in the layer waits for the matrix, and up to N = 4096 its write
 * shares ONE launch with the per-image chain (masked groups: K3..K6; unmasked: up to the group structure, the per-group
 * solves and K6 follow).  N > 4096 (masked groups): the write runs beside the layer on the library's side stream (see
 * Conventions).  The ungrouped mode builds its pruned triangular matrix from the boxes as well; only pre-sorted scores
 * read the matrix back.  gnms_backward pairs with it unchanged (grouped unmasked: gnms_backward_from_boxes does too, and
 * never reads the matrix). */
int gnms_forward_with_iou2d(const float* boxes, const float* scores, int B, int N, int64_t ld, const int32_t* counts,
                            const gnms_params* params, float* iou_out, float* prob, int64_t* order, int64_t* valid,
                            int64_t* invalid, int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The same for the 3D overlap of lib/loss/rpn_3d.py:778-784 (overlap_in_nms == "3d"): params3d [B][N][7] = x y z w h l ry ->
 * iou_out [B][N][ld] = 0.5 * (1 + GIoU3D) (as gnms_nms_overlap3d_from_params with params->nms_threshold) -> the outputs of gnms_forward.  Grouped + masked
 * hard-sort modes take the threshold bits and the single group overlaps from the cuboid records with the arithmetic that wrote
 * the matrix (no read-back of the 4 N^2 bytes; N > 4096: matrix write on the side stream); the other modes read the matrix.
 * gnms_backward pairs with it unchanged. */
int gnms_forward_with_iou3d(const float* params3d, const float* scores, int B, int N, int64_t ld, const int32_t* counts,
                            const gnms_params* params, float* iou_out, float* prob, int64_t* order, int64_t* valid,
                            int64_t* invalid, int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The two per-image counts of a forward call on the HOST: what the reference's return convention needs before it can shape
 * `valid_boxes_index` / `invalid_boxes_index` (lib/groomed_nms.py:120-127; their length K is data dependent).  Blocking; ordered behind
 * everything enqueued on `stream` before it.  nvalid / ninvalid: the DEVICE arrays [B] a gnms_forward* call wrote; host_out: HOST array
 * [2 B] = nvalid[0..B) then ninvalid[0..B).  Not a device-to-host copy: a one-wave kernel stores the counts and a call tag into a slot of
 * fine-grained pinned memory the library keeps per device (64 KiB, allocated by the first call) and the host polls the tag (one PCIe
 * write instead of a copy submission + a stream synchronisation: ~20 us less per call at N = 500).  B > 127, or no tag within two
 * seconds: a plain asynchronous copy + stream synchronisation.  Cannot be captured into a graph (GNMS_ERR_INVALID_ARGUMENT). */
int gnms_counts_to_host(const int32_t* nvalid, const int32_t* ninvalid, int B, int32_t* host_out, void* stream);
/* The same trip without any launch behind the layer: gnms_host_counts_slot hands out 2 B words of that pinned memory, preset to -1, as the
 * device (`device_view`) and the host (`host_view`) address them; pass device_view as `nvalid` and device_view + B as `ninvalid` to ONE
 * gnms_forward* call (the kernels store each count exactly once, at the end of the image's chain), then gnms_host_counts_wait polls
 * host_view until all 2 B words are counts (>= 0) and copies them to host_out [2 B]; it falls back to a stream synchronisation when the
 * stream runs empty first or after two seconds.  B <= 127 (GNMS_ERR_UNSUPPORTED above).
 * OWNERSHIP: the slot belongs to the caller from gnms_host_counts_slot until gnms_host_counts_wait returns (whatever it returns) or
 * gnms_host_counts_release is called -- exactly one of the two per slot; nobody else is handed the slot in between, however many calls other
 * threads make on the device.  When all 64 slots of the device are owned, gnms_host_counts_slot returns GNMS_ERR_UNSUPPORTED and the caller
 * takes the plain path (device counts + gnms_counts_to_host).  gnms_host_counts_release is for a caller that took a slot and will not wait
 * (its forward call failed, or was never made): it synchronises `stream` first, so a forward call that was enqueued can no longer store
 * into a slot somebody else owns by then.  A wait / release on a view that is not owned is GNMS_ERR_INVALID_ARGUMENT.
 * differentiable_nms at N = 500, index tensors included: 64 -> 46 us per call. */
int gnms_host_counts_slot(int B, int32_t** device_view, const int32_t** host_view);
int gnms_host_counts_wait(const int32_t* host_view, int B, int32_t* host_out, void* stream);
int gnms_host_counts_release(const int32_t* host_view, void* stream);
/* test hook: the number of mailbox slots gnms_host_counts_slot / gnms_counts_to_host may use per device (1 .. 64); returns the previous value */
int gnms_test_mailbox_slots(int n);

/* backward of L through prob.  grad_prob [B][N] = dL/dprob (same order as prob).
 *   grad_scores [B][N] (input order), overwritten.
 *   grad_iou    [B][N][ld] or NULL.  When given it is fully overwritten (zero fill + the sparse
 *               entries); training detaches the matrix (lib/loss/rpn_3d.py:791), so NULL is the fast path.
 * scores/iou/counts/params/workspace must be the ones the forward call saw. */
int gnms_backward(const float* grad_prob, const float* scores, const float* iou, int B, int N, int64_t ld,
                  const int32_t* counts, const gnms_params* params, float* grad_scores, float* grad_iou,
                  void* workspace, size_t workspace_bytes, void* stream);

/* From-boxes path (2D): the same layer computed straight from boxes [B][N][4] = (x1,y1,x2,y2); the N x N overlap
 * matrix is never materialised -- the bit-matrix kernel recomputes every pair's IoU in registers with the arithmetic of
 * gnms_iou2d (lib/core.py:499-508), so all outputs and gradients are bit-identical to gnms_iou2d + gnms_forward /
 * gnms_backward.  Grouped, hard-sorted modes only (masked or unmasked groups); ungrouped / presorted return
 * GNMS_ERR_UNSUPPORTED (they need the matrix).  HBM traffic drops from 8 N^2 to N^2/8 + O(N) bytes per image; the
 * bound becomes fp32 VALU.  Workspace: gnms_workspace_bytes. */
int gnms_forward_from_boxes(const float* boxes, const float* scores, int B, int N, const int32_t* counts,
                            const gnms_params* params, float* prob, int64_t* order, int64_t* valid, int64_t* invalid,
                            int32_t* nvalid, int32_t* ninvalid, void* workspace, size_t workspace_bytes, void* stream);
int gnms_backward_from_boxes(const float* grad_prob, const float* boxes, const float* scores, int B, int N,
                             const int32_t* counts, const gnms_params* params, float* grad_scores, void* workspace,
                             size_t workspace_bytes, void* stream);

/* backward of L through prob WITH the gradient w.r.t. the 2D boxes the overlaps were computed from (iou = gnms_iou2d(boxes, boxes)):
 * what autograd gives the reference for differentiable_nms(scores, iou(boxes, boxes)) when the caller does not detach.  Pairs with
 * every 2D forward entry (gnms_forward on that matrix, gnms_forward_with_iou2d, gnms_forward_from_boxes); scores / counts / params /
 * workspace must be the ones the forward call saw.
 *   grad_scores [B][N], grad_boxes [B][N][4] (input order), both fully overwritten; boxes behind counts[b] and boxes in no group get 0.
 *   iou         the forward's matrix [B][N][ld], or NULL: the dense route then rebuilds it in `scratch` (ld is its row stride there too).
 *   route       GNMS_BOXES_ROUTE_AUTO: masked groups, hard sort, unsorted output (the default mode) take the SPARSE route -- the matrix
 *               gradient has one entry per non-head member, so the members' and heads' box gradients come out of one O(N) launch
 *               behind gnms_backward's, no N x N pass, no scratch, `iou` not read.  Every other mode, and GNMS_BOXES_ROUTE_DENSE for
 *               any mode: gnms_backward with grad_iou written into `scratch`, then gnms_iou2d_backward with the boxes on both sides.
 *   scratch     gnms_backward_boxes_scratch_bytes(B, N, ld, params, iou != NULL, route) bytes, 256-byte aligned (0 on the sparse route).
 * A non-head member's gradient is the same bits on both routes (one term); a head's is a sum in member order on the sparse route. */
#define GNMS_BOXES_ROUTE_AUTO 0
#define GNMS_BOXES_ROUTE_DENSE 1
size_t gnms_backward_boxes_scratch_bytes(int B, int N, int64_t ld, const gnms_params* params, int have_iou, int route);
int gnms_backward_boxes(const float* grad_prob, const float* boxes, const float* scores, int B, int N, const int32_t* counts,
                        const gnms_params* params, float* grad_scores, float* grad_boxes, const float* iou, int64_t ld, int route,
                        void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* What the backward of a forward call will read besides scores / counts / workspace -- the ONE place a binding learns what to keep alive
 * between the two calls and which gnms_backward* entry follows.  Pure host code: no HIP call, no launch, no device needed.  It answers
 * from the same gate definitions the entries themselves branch on (nms_layer.hip).
 *   entry           the forward entry, GNMS_ENTRY_*
 *   boxes           the pointer that entry gets as boxes / params3d (only its 16-byte alignment is looked at); NULL for GNMS_ENTRY_MATRIX
 *   box_grad_route  GNMS_BOXES_ROUTE_NONE: gnms_backward, or with GNMS_BWD_FROM_BOXES gnms_backward_from_boxes, follows;
 *                   GNMS_BOXES_ROUTE_AUTO / _DENSE: gnms_backward_boxes follows with that route (the two 2D one-call entries only)
 * Returns GNMS_BWD_* flags (>= 0), or a negative gnms status with gnms_last_error set (unknown entry / route, NULL params, NULL boxes
 * where the entry takes some).  `masked` = group_boxes && mask_group_boxes; `default` = masked && !return_sorted_prob && !presorted:
 *
 *   no box gradient      mode                                                      flags
 *   ENTRY_MATRIX         every mode                                                READS_MATRIX  (the caller's own tensor; masked groups read
 *                                                                                                 it only for grad_iou, and keeping it costs nothing)
 *   ENTRY_WITH_IOU2D     masked                                                    0             (the matrix is free to be overwritten at once)
 *                        group_boxes, unmasked, !presorted, boxes 16-byte aligned  READS_BOXES | FROM_BOXES  (the forward ran from the boxes too)
 *                        everything else (ungrouped; presorted; an unaligned view) READS_MATRIX  (the forward itself refuses an unaligned view
 *                                                                                                 as things stand: its gnms_iou2d does)
 *   ENTRY_WITH_IOU3D     masked                                                    0
 *                        everything else                                           READS_MATRIX
 *   ENTRY_FROM_BOXES     every mode it accepts                                     READS_BOXES | FROM_BOXES
 *
 *   box gradient         route AUTO and default mode (the sparse route)            READS_BOXES
 *                        route DENSE, or any other mode                            READS_BOXES | READS_MATRIX  (pass the forward's matrix as `iou`
 *                                                                                                 where the entry wrote one, else NULL)
 *                        + boxes not 16-byte aligned                               | COPY_BOXES
 *
 * The cuboid gradient behind GNMS_ENTRY_WITH_IOU3D is not a row of this table (a box-gradient route with that entry stays an error
 * here): ask its sibling, gnms_backward_cuboids_reads, below.
 */
#define GNMS_ENTRY_MATRIX 0     /* gnms_forward */
#define GNMS_ENTRY_WITH_IOU2D 1 /* gnms_forward_with_iou2d */
#define GNMS_ENTRY_WITH_IOU3D 2 /* gnms_forward_with_iou3d */
#define GNMS_ENTRY_FROM_BOXES 3 /* gnms_forward_from_boxes */
#define GNMS_BOXES_ROUTE_NONE -1
#define GNMS_BWD_READS_MATRIX 1 /* the backward reads the overlap matrix the forward read or wrote */
#define GNMS_BWD_READS_BOXES 2  /* the backward reads the boxes */
#define GNMS_BWD_FROM_BOXES 4   /* the backward entry is gnms_backward_from_boxes */
#define GNMS_BWD_COPY_BOXES 8   /* gnms_backward_boxes and the forward in front of it load a box as one float4: give BOTH a 16-byte aligned copy */
int gnms_backward_reads(int entry, const gnms_params* params, const void* boxes, int box_grad_route);

/* backward of L through prob WITH the gradient w.r.t. the cuboids params3d [B][N][7] the 3D NMS overlap was computed from: what autograd
 * gives the reference for differentiable_nms(scores, 0.5 (1 + iou3d_approximate(corners(params), "generalized"))) when the caller does
 * not detach.  Pairs with gnms_forward_with_iou3d (and with gnms_forward on gnms_nms_overlap3d_from_params' matrix at
 * params->nms_threshold); scores / counts / params / workspace must be the ones the forward call saw.
 *   grad_scores [B][N], grad_params3d [B][N][7] (input order), both fully overwritten; boxes behind counts[b] and boxes in no group get 0.
 *   overlap     the forward's matrix [B][N][ld], or NULL: the dense route then rebuilds it in `scratch` with the forward's own writer
 *               (gnms_nms_overlap3d_from_params at params->nms_threshold; that call allocates stream-ordered).
 *   route       GNMS_BOXES_ROUTE_AUTO in the default mode: the SPARSE route -- gnms_backward, then one O(N) launch (a member's row is
 *               one term, a head's row a sum over its run in member order), no N x N pass, no scratch, `overlap` not read; the
 *               member's cotangent is (-(gx s_head)) f'(q) with q the matrix entry as the forward defines it (guard band included).
 *               Every other mode, and GNMS_BOXES_ROUTE_DENSE for any mode: gnms_backward with grad_iou written into `scratch`, then
 *               gnms_iou3d_backward (method 2) with the cuboids on both sides.
 *   scratch     gnms_backward_cuboids_scratch_bytes(B, N, ld, params, overlap != NULL, route) bytes, 256-byte aligned (0 on the sparse route).
 * A non-head member's gradient is the same bits on both routes (one term); a head's is a sum in member order on the sparse route.
 * gnms_backward_cuboids_reads (host code only, the same gates): GNMS_BWD_READS_BOXES on the sparse route, GNMS_BWD_READS_BOXES |
 * GNMS_BWD_READS_MATRIX otherwise; never COPY_BOXES (a 28-byte row is not loaded as a float4); negative with gnms_last_error set for
 * NULL params / params3d or an unknown route. */
size_t gnms_backward_cuboids_scratch_bytes(int B, int N, int64_t ld, const gnms_params* params, int have_overlap, int route);
int gnms_backward_cuboids(const float* grad_prob, const float* params3d, const float* scores, int B, int N, const int32_t* counts,
                          const gnms_params* params, float* grad_scores, float* grad_params3d, const float* overlap, int64_t ld, int route,
                          void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gnms_backward_cuboids_reads(const gnms_params* params, const void* params3d, int route);

/* profiling hook: re-runs only the threshold bit-matrix kernel (the single full read of the overlap matrix, the
 * dominant kernel of gnms_forward) on a workspace a previous gnms_forward call filled. */
int gnms_profile_bitmask(const float* iou, int B, int N, int64_t ld, const int32_t* counts, float nms_threshold,
                         void* workspace, size_t workspace_bytes, void* stream);

/* same hook for the from-boxes bit-matrix kernel (VALU bound) */
int gnms_profile_bitmask_boxes(const float* boxes, int B, int N, const int32_t* counts, float nms_threshold, void* workspace,
                               size_t workspace_bytes, void* stream);

/* profiling / test hook: only the sorts in front of the 2D layer (scores descending; with `boxes` [B][N][4], which may be NULL, also the
 * boxes by x centre), on a chosen route: 0 = what the layer takes, 1 = runs + merge (two launches), 2 = ranked runs and 3 = by histogram
 * (one launch each, 2048 < N <= 4096, GNMS_ERR_UNSUPPORTED elsewhere).  What the sorts leave in the workspace is copied into the caller's arrays, each
 * [B][N] (rbox, xbox: [B][N][4]) and each optional: order, rankof, sscore, and with boxes rbox, xidx, xbox (zeros behind an image's
 * count); flags [B][2] = "the scores came in sorted", "some box is not plain". */
int gnms_profile_sorts(const float* scores, const float* boxes, int B, int N, const int32_t* counts, int route, int32_t* order,
                       int32_t* rankof, float* sscore, float* rbox, int32_t* xidx, float* xbox, int32_t* flags, void* workspace,
                       size_t workspace_bytes, void* stream);

/* test hook: how the histogram sort (route 3, and route 0 where the layer takes it) went in the last call on this workspace.  paths: device
 * array [B][2] (role 0 = scores, role 1 = boxes), 1 = ranked by histogram, 2 = some bin held more than the cap and the image and role fell
 * back to the run sort; the slot is written by that kernel only, so after another route it holds what was there before.  cap_out (host,
 * optional): the cap, keys in one bin, that later calls use. */
int gnms_profile_sort_paths(int B, int N, int32_t* paths, int32_t* cap_out, void* workspace, size_t workspace_bytes, void* stream);

/* developer hook (the cap series of tools/sort_routes.py): the histogram sort's cap for later calls, process-wide; 0 = every image falls
 * back, 769 (the largest; more is clamped to it) = only bins past 769 keys do, negative = the built-in value.  Returns the previous cap. */
int gnms_profile_set_hist_cap(int cap);

/* Per-launch timing of the two HBM-bound launches inside whatever call sequence the caller runs (bench.py's roofline line).
 * gnms_profile_events(1) arms it: from then on every launch that writes an N x N overlap matrix (slot GNMS_PROF_MATRIX_WRITE:
 * gnms_iou2d, gnms_iou3d_*, gnms_forward_with_iou2d / _iou3d), every launch of the kernel that reads one (slot GNMS_PROF_MATRIX_READ:
 * gnms_forward's bit-matrix kernel) and the plain streams below (slot GNMS_PROF_PLAIN_STREAM) go through hipExtLaunchKernel with a
 * start and a stop event -- the dispatch's own begin / end timestamps, what a kernel trace reports, no marker packet in the stream.
 * Not capturable in a HIP graph; one profiling thread at a time.  gnms_profile_collect waits for the recorded events
 * and returns the SUM of the launch durations (ms) and their number since the last collect.  gnms_profile_events(0) disarms.
 * gnms_profile_fill / gnms_profile_read: a plain non-temporal float4 store / load stream over `count` floats -- the HBM write /
 * read rate a kernel that does nothing else reaches on this device (the ceiling the roofline fraction is quoted beside). */
#define GNMS_PROF_MATRIX_WRITE 0
#define GNMS_PROF_MATRIX_READ 1
#define GNMS_PROF_PLAIN_STREAM 2
int gnms_profile_events(int enable);
int gnms_profile_collect(int slot, double* ms_sum, int* launches);
const char* gnms_profile_write_kernel_name(int dim, int B, int N); /* the launch that writes the matrix in gnms_forward_with_iou2d (dim 2) / _iou3d (dim 3), as a kernel trace names it */
int gnms_profile_fill(float* dst, size_t count, void* stream);
int gnms_profile_fill_tiles(float* dst, int B, int N, int64_t ld, int rows, int nontemporal, void* stream);
/* the store pattern of a symmetric matrix writer, no arithmetic: upper-triangular tile x tile macro tiles (tile = 128 or 256, dividing
 * N), each written where it is and mirrored; cols_per_lane 2 or 4 floats per lane and store instruction; persist: one workgroup per
 * CU (two at tile 128) walks a contiguous range of tiles, else one workgroup per tile.  Timed like gnms_profile_fill. */
int gnms_profile_fill_sym(float* dst, int B, int N, int64_t ld, int tile, int cols_per_lane, int nontemporal, int persist, void* stream); /* the same store stream in the matrix writers' geometry: persistent 16-wave workgroups, `rows` (4, 8, 16, 32 or 64, dividing N) rows x 1 KiB per wave, rows ld floats apart; non-temporal (as the writers store) or ordinary 16-byte stores */
int gnms_profile_read(const float* src, size_t count, float* sink, void* stream);

/* get_groups(iou_unsorted, group_threshold, scores_unsorted, group_size)  lib/groomed_nms.py:208-270 for one
 * image.  group_of[N]: index of the box's group (groups numbered in creation order) or -1 if the box is in
 * no group (beyond the cap, or NaN overlap with its leader); pos_in_group[N]: position inside the group
 * (0 = first member).  Both int32, indexed by INPUT index.  *ngroups_out is a device int32. */
int gnms_get_groups(const float* scores, const float* iou, int N, int64_t ld, float group_threshold, int group_size,
                    int32_t* group_of, int32_t* pos_in_group, int32_t* ngroups_out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* pruning_function(iou, nms_threshold, temperature, pruning_method)  lib/groomed_nms.py:167-189, elementwise */
int gnms_pruning_function(const float* iou, int64_t count, float nms_threshold, float temperature, int pruning_method,
                          float* out, void* stream);
/* its adjoint (the reference differentiates the same expressions with autograd): grad_iou[i] = grad_out[i] * f'(iou[i]) */
int gnms_pruning_function_backward(const float* iou, const float* grad_out, int64_t count, float nms_threshold, float temperature,
                                   int pruning_method, float* grad_iou, void* stream);

/* soft_sort(scores, full_matrix, temperature)  lib/groomed_nms.py:131-165 for one image.
 * C [N][N] (convex_comb_matrix, including the reference's last-axis broadcast of the row sums, :155),
 * soft_scores [N] = C s, soft_matrix [N][N] = C iou (fp32 MFMA GEMM).  iou/soft_matrix may both be NULL. */
int gnms_soft_sort(const float* scores, const float* iou, int N, int64_t ld, float temperature, float* C,
                   float* soft_scores, float* soft_matrix, void* workspace, size_t workspace_bytes, void* stream);

/* Adjoint of gnms_soft_sort (the reference differentiates lib/groomed_nms.py:145-164 with autograd).  scores, temperature, C and
 * `workspace` are what the forward call saw / produced (the workspace still holds the sorted scores, their order and the row sums);
 * matrix [N][ld] with K columns is the matrix that was multiplied (NULL: none).  Upstream gradients, each may be NULL: g_soft [N]
 * (of soft_scores), g_C [N][N] (of C), g_mat [N][K] (of soft_matrix).  Outputs: d_scores [N]; d_matrix [N][ld] or NULL.
 * scratch: gnms_soft_sort_backward_scratch_bytes(N, K) bytes, 16-byte aligned.  The two products (g_mat M^T, C^T g_mat) run on
 * the MFMA GEMM; row and column passes are deterministic (no atomics). */
size_t gnms_soft_sort_backward_scratch_bytes(int N, int K);
int gnms_soft_sort_backward(const float* scores, const float* matrix, int N, int K, int64_t ld, float temperature, const float* C,
                            const float* g_soft, const float* g_C, const float* g_mat, float* d_scores, float* d_matrix,
                            void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* D[M x N] = A[M x K] B[K x N], fp32 row-major with leading dimensions lda/ldb/ldd, on the matrix cores
 * (v_mfma_f32_32x32x2_f32: exact fp32, an fmaf chain over k).  The GEMM behind soft_sort's C @ iou (:163).  Small problems (fewer
 * than two 128 x 128 tiles per CU) split K over up to 16 slices: a stream-ordered temporary of slices x M x N floats, the slices
 * summed in order (deterministic; a different association of the same sum). */
int gnms_sgemm(const float* A, const float* B, float* D, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldd,
               void* stream);
/* Round 6: from 512 x 512 x 512 on the PLAIN product runs on rocBLAS, from 2048^3 on on hipBLASLt, when the library can be found (dlopen at
 * first use; a stream that is being captured keeps the kernels of this library), see csrc/soft_sort.hip.  gnms_profile_sgemm picks the path
 * for comparisons: variant 0 = what gnms_sgemm does, 1 = this library's MFMA kernels only, 2 = rocBLAS only, 4 = hipBLASLt only
 * (GNMS_ERR_UNSUPPORTED when it is missing), 3 = variant 1 with the large kernel's workgroups de-phased (a measured experiment). */
int gnms_profile_sgemm(const float* A, const float* B, float* D, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldd,
                       int variant, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Classical hard NMS (lib/nms)
 * ------------------------------------------------------------------------------------------- */

/* EXACT reference symbol and contract (lib/nms/gpu_nms.hpp:1-2, lib/nms/nms_kernel.cu:91-144):
 * host pointers, boxes_host is boxes_num x boxes_dim fp32 pre-sorted by descending score,
 * keep_out holds boxes_num ints, blocking.  +1-pixel IoU (:24-32), strict '>' (:71).
 * boxes_num <= GNMS_MAX_BOXES runs the layer's leader scan (one workgroup per super-block); larger inputs -- the reference's `use_nms and
 * synced` inference branch (lib/rpn_util.py:1268) feeds every anchor, > 100 k -- are processed in chunks of GNMS_MAX_BOXES (round 6): what the
 * boxes kept so far suppress in the chunk straight from the boxes, the chunk's own bit matrix, the same scan, the kept boxes appended -- the
 * reference's keep list with n^2 / (2 chunks) + n * kept pair decisions and 33 MB of device memory where the n x n mask is 2 GB at 126 720
 * boxes.  Limit: boxes_num <= 262144; above it *num_out = 0 and gnms_last_error() says so (the Python wrapper gpu_nms raises). */
void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
          float nms_overlap_thresh, int device_id);

/* device-pointer, stream-ordered variant: boxes [n][boxes_dim] sorted by score; keep [n] int32; num_out device int32.
 * workspace: gnms_nms_workspace_bytes(n). */
size_t gnms_nms_workspace_bytes(int n);
int gnms_nms_sorted(const float* boxes, int n, int boxes_dim, float thresh, int32_t* keep, int32_t* num_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* the same scan with the pixel convention and the comparison as parameters: areas and overlaps use (x2 - x1 + shift); keep_le = 0
 * suppresses when IoU > thresh (`_nms`), keep_le = 1 keeps only IoU <= thresh -- lib/nms_others.py:119-150 girshick_nms(dets, thresh,
 * shift) on score-sorted boxes (a NaN overlap then suppresses, as `np.where(ovr <= thresh)` does). */
int gnms_nms_sorted_shift(const float* boxes, int n, int boxes_dim, float thresh, float shift, int keep_le, int32_t* keep,
                          int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream);
/* the same for float64 boxes, every operation in double: girshick_nms computes in the dtype of `dets` (lib/nms_others.py:119-150),
 * float64 for the arrays the reference's own test feeds it (test/test_differentiable_nms_forward.py:111-114) */
int gnms_nms_sorted_shift_f64(const double* boxes, int n, int boxes_dim, double thresh, double shift, int keep_le, int32_t* keep,
                              int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream);

/* lib/nms_others.py:6-116 navneeth_soft_nms(boxes, sigma, Nt, threshold, method, shift): Soft-NMS with the reference's slot
 * bookkeeping.  boxes [n][boxes_dim] (x1 y1 x2 y2 score ...), fp64 when is_fp64 else fp32, NOT modified (the reference decays the
 * scores and swaps the rows of its argument in place).  method 0 hard, 1 linear, 2 gaussian.  keep [n] int64: the kept ORIGINAL
 * indices in the reference's slot order (`keep_orig[:N]`), *num_out (device int32) of them.  One workgroup; n <= GNMS_MAX_BOXES.
 * workspace: gnms_soft_nms_workspace_bytes(n), 256-byte aligned. */
size_t gnms_soft_nms_workspace_bytes(int n);
int gnms_soft_nms(const void* boxes, int n, int boxes_dim, int is_fp64, double sigma, double Nt, double threshold, int method, double shift,
                  int64_t* keep, int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * After-NMS AP loss (lib/loss/aploss.py:14-87 backpropAPLoss.forward, called per image on the rescored
 * scores at lib/loss/rpn_3d.py:1117-1131): the immediate consumer of gnms_forward's `prob`.
 *   logits, targets: [B][N] fp32 (image b uses its first counts[b] entries, all N when counts is NULL).
 *   loss: [B] = 1 - mean precision of the positives; grad: [B][N] = d loss / d logits, both produced by the
 *   forward pass as in the reference (:69-78; its backward only scales grad by the incoming gradient, :80-85).
 *   An image without a positive (max(targets) <= 0, :26-28) gets loss 0 and a zero gradient.
 *   delta is 1.0 whatever the caller of the reference passes (:16).  N <= GNMS_MAX_BOXES.  Up to 2047 boxes per image one workgroup per
 *   image does everything in LDS (no scratch); larger images take a stream-ordered temporary of 8 N words per image and spread the
 *   positives over the machine (four launches).
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_APLOSS_MAX_BOXES GNMS_MAX_BOXES
int gnms_aploss(const float* logits, const float* targets, int B, int N, const int32_t* counts, float positive_label,
                float negative_label, float* loss, float* grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * In front of the layer: decode and selection of the boxes the NMS sees, on the device.
 * ------------------------------------------------------------------------------------------------ */
/* lib/rpn_util.py:872-934 bbox_transform_inv.  anchors [A][4] (x1 y1 x2 y2), deltas [B][A][4] (dx dy dw dh; NOT modified,
 * the reference scales its argument in place, :903-913), means / stds: HOST pointers to 4 floats or NULL; out [B][A][4]. */
int gnms_bbox_transform_inv(const float* anchors, const float* deltas, int B, int A, const float* means, const float* stds,
                            float* out, void* stream);
/* lib/loss/rpn_3d.py:731-737 (and lib/rpn_util.py:1258-1266): per image the candidates' scores sorted descending (stable: ties
 * keep candidate order), the first min(K, #candidates) selected.  scores [B][A]; candidates [B][F] int32 indices into [0, A)
 * with candidate_counts [B] (NULL: all F), or candidates == NULL: every one of the A boxes is a candidate.  More than GNMS_MAX_BOXES
 * candidates (all ~127k anchors of an image at inference): a radix pre-selection first leaves exactly the K the stable sort would put
 * first (then K <= GNMS_MAX_BOXES; a stream-ordered temporary of B * (K + 1) ints).  From 4096 candidates on, while B * ceil(F / 8192)
 * workgroups fit the device and the stream is not being captured, several workgroups per image do the selection together: they use ONE
 * scratch per device that the library keeps between the calls (about 12 MiB + 16 bytes per selected box; grown with a blocking
 * hipFree / hipMalloc when a call needs more), and launches of that kind are ordered across streams by an event per device.
 * Outputs (any may be NULL), padded behind sel_count[b]: sel_index [B][K] int64 (-1), sel_scores [B][K] (0),
 * sel_boxes [B][K][4] gathered from boxes [B][A][4] (0) -- the padded layout gnms_forward_with_iou2d takes with counts. */
int gnms_select_topk(const float* scores, int B, int A, const int32_t* candidates, int F, const int32_t* candidate_counts, int K,
                     const float* boxes, int64_t* sel_index, int32_t* sel_count, float* sel_scores, float* sel_boxes, void* stream);
/* lib/loss/rpn_3d.py:746-768 ("projected" 2D boxes): params [B][N][7] = x y z w h l ry -> cuboid corners (lib/math_3d.py:364-435)
 * -> projected with p2 [B][16] (4x4 row-major, lib/math_3d.py:47-72) -> min/max over the corners -> times scale[b] (NULL: 1). */
int gnms_project_boxes3d(const float* params, const float* p2, const float* scale, int B, int N, float* boxes2d, void* stream);

/* lib/loss/rpn_3d.py:801-825: the best box per ground truth after the NMS.
 * score[i][j] = 0.5 * (1 + GIoU3D(pred_i, gt_j)) * IoU2D(pred_i, gt_j); best[j] = first argmax over the predictions, kept if
 * score > beta (self.best_target_box_beta); targets[b][best] = 1, everything else 0.
 * pred_params [B][N][7], gt_params [B][M][7] = x y z w h l ry; pred_boxes2d [B][N][4], gt_boxes2d [B][M][4]; counts NULL = all.
 * Outputs (any may be NULL): best_index [B][M] int64 (-1: none / below beta), best_score [B][M], targets [B][N] fp32. */
int gnms_best_targets(const float* pred_params, const float* pred_boxes2d, const float* gt_params, const float* gt_boxes2d, int B, int N,
                      int M, const int32_t* pred_counts, const int32_t* gt_counts, float beta, int64_t* best_index, float* best_score,
                      float* targets, void* stream);

/* lib/rpn_util.py:411-524 compute_targets (and lib/core.py:535 iou_ign) for B images: the anchor training targets of the RPN loss
 * (lib/loss/rpn_3d.py:435-451), on the device.  DESIGN.md 3.10 has the passes and the precision rules.
 * rois [B][R][ld_rois] x1 y1 x2 y2 (+ the anchor tracker in column tracker_col), float32 or (rois_f64) float64; the arithmetic that
 * involves a roi alone is done in that type, everything that involves a ground truth in float64, as NumPy's promotion does.
 * gts_val [B][M][4] with box_lbls [B][M] (>= 1) and gts_ign [B][K][4], float64 x1 y1 x2 y2; image b uses the first val_counts[b] /
 * ign_counts[b] rows (device int32, NULL = all; clamped to [0, M] / [0, K]); padding rows are never read.  M, K <= GNMS_TARGETS_MAX_GTS
 * (GNMS_ERR_UNSUPPORTED above).  gts_3d [B][M][D3] float64 with 7 <= D3 <= GNMS_TARGETS_MAX_D3, or D3 = 0: 2D only.  D3 alone sets
 * the output widths; gts_3d may be NULL when M = 0.
 * anchor_cols sets decomp_alpha (>= 11) and has_vel (== 12) as anchors.shape[1] does (0: neither); src_3d = rois_3d[:, 4:]
 * ([B][R][ld_rois_3d], rois_3d_f64) or, with rois_3d NULL, anchors[int64(rois[:, tracker_col]), 4:] (anchors [A][anchor_cols] float64;
 * a tracker outside [-A, A) gives NaN deltas).  rois_3d_cen [B][R][2] (cen_f64) or NULL: the 3D centre deltas' origin.
 * means_host / stds_host: NULL or 4 + (decomp ? 9 : 7) float64 (4 with D3 = 0): the call site's normalisation, fused.
 * Outputs, each optional (NULL), all written on every call (no reliance on zeroed buffers): transforms [B][R][5 + D3 + 2 decomp + vel]
 * ([B][R][5] with D3 = 0), raw_gt [B][R][5 + D3] ([B][R][5]), float32; ols_max [B][R], ols [B][R][M] (IoU, columns past the
 * image's count 0), ols_ign [B][R][K] (iou_ign, likewise), float64; best_roi [B][M] int64, the roi each GT keeps (-1: none).
 * workspace: gnms_compute_targets_workspace_bytes(B, R, M) bytes (8-byte aligned; 12 bytes per GT and image per 256 rois), every
 * byte of it written before it is read.  Two launches, no atomics, no allocation: graph-capturable. */
#define GNMS_TARGETS_MAX_GTS 256
#define GNMS_TARGETS_MAX_D3 24
size_t gnms_compute_targets_workspace_bytes(int B, int R, int M);
int gnms_compute_targets(const void* rois, int rois_f64, int B, int R, int64_t ld_rois, const double* gts_val, const int32_t* box_lbls,
                         int M, const int32_t* val_counts, const double* gts_ign, int K, const int32_t* ign_counts, const double* gts_3d,
                         int D3, const void* rois_3d, int rois_3d_f64, int64_t ld_rois_3d, const void* rois_3d_cen, int cen_f64,
                         const double* anchors, int A, int anchor_cols, int tracker_col, double fg_thresh, double ign_thresh,
                         double bg_thresh_lo, double bg_thresh_hi, double best_thresh, const double* means_host, const double* stds_host,
                         float* transforms, float* raw_gt, double* ols_max, double* ols, double* ols_ign, int64_t* best_roi,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference post-processing of the detection head (lib/rpn_util.py:1087-1356, im_detect_3d between `net(im)` and the returned
 * `aboxes`), around gnms_select_topk and the NMS routes above.  Three stream-ordered launches, no allocation, no workspace:
 * graph-capturable.  The selection comes BEFORE the decode: only the scores pass touches all A anchors.
 * ------------------------------------------------------------------------------------------------ */
/* :1193-1194, :1256.  prob [B][A][C] (column 0 = background, C >= 2), acceptance NULL or [B][A][acceptance_ld] (column 0 is read)
 * -> scores [B][A] = max(prob[1:]) (* acceptance: one fp32 product, as the reference's), cls_pred [B][A] = argmax(prob[1:]) + 1,
 * first maximum on ties, a NaN counts as the maximum (np.argmax / np.amax). */
int gnms_detect3d_scores(const float* prob, const float* acceptance, int64_t acceptance_ld, int B, int A, int C, float* scores,
                         int32_t* cls_pred, void* stream);
/* :1111-1170, :1182-1215 for the selected anchors.  sel_index [B][ld_index] (the first K of a row are read; gnms_select_topk's
 * output), counts [B] or NULL (all K); entries behind an image's count are written as zeros.  bbox_2d [B][A][4], bbox_3d [B][A][D3]
 * (D3 >= 10 with decomp_alpha: x y z w h l rsin rcos axis head; else >= 7: ... ry), rois [A][5] (x1 y1 x2 y2 tracker), anchors
 * [n_anchors][anchor_cols] fp32 (columns 4.. = z w h l ry [sin cos]; a tracker outside [0, n_anchors) is clamped), means_host /
 * stds_host: HOST pointers to norm_cols floats (4 for the 2D box alone, 11 / 13 with the 3D outputs), p2_inv [B][4][4] float64 (needed
 * for coords_3d_raw only), scale_factor [B] or NULL (1).
 * Outputs, each optional: boxes2d [B][K][4] = bbox_transform_inv(rois, bbox_2d, means, stds)[sel] / scale_factor, the arithmetic of
 * gnms_bbox_transform_inv (shared device code) and an fp32 division; coords_3d [B][K][7] = x y (pixels, / scale_factor) z w h l alpha,
 * fp32 in the reference's operation order, not wrapped; coords_3d_raw [B][K][7] = the camera-space x y z through p2_inv in float64
 * (from the fp32 products x z and y z), w h l, and rotation_y = alpha + atan2(-z, x) + pi / 2 wrapped into (-pi, pi] in float64
 * (lib/util.py:641-644), all rounded to fp32. */
int gnms_detect3d_decode(const int64_t* sel_index, int64_t ld_index, const int32_t* counts, int B, int K, int A, const float* bbox_2d,
                         const float* bbox_3d, int D3, const float* rois, const float* anchors, int n_anchors, int anchor_cols,
                         const float* means_host, const float* stds_host, int norm_cols, int decomp_alpha, const double* p2_inv,
                         const float* scale_factor, float* boxes2d, float* coords_3d, float* coords_3d_raw, void* stream);
/* :1338-1351.  keep [B][ld_keep]: positions in [0, K) of the kept boxes in output order (int64 when keep_is_i64 -- the layer's `valid`
 * lists --, int32 otherwise -- gnms_nms_sorted's keep list; NULL: 0, 1, 2, ...), keep_counts [B] (NULL: K).  sel_scores [B][ld_scores]
 * and sel_index [B][ld_index] from gnms_select_topk, cls_pred [B][A] from gnms_detect3d_scores, boxes2d [B][K][4] and coords_3d
 * [B][K][7] from gnms_detect3d_decode, rois [A][5].  clip_hw NULL or [B][2] = (height, width) of the original image: x clipped to
 * [0, width - 1], y to [0, height - 1] (rpn_conf.clip_boxes).  out [B][K][14] = x1 y1 x2 y2 score cls coords_3d[7] tracker, rows
 * behind the image's count zero; out_counts [B] (optional). */
int gnms_detect3d_assemble(const void* keep, int keep_is_i64, int64_t ld_keep, const int32_t* keep_counts, const float* sel_scores,
                           int64_t ld_scores, const int64_t* sel_index, int64_t ld_index, const int32_t* cls_pred, const float* boxes2d,
                           const float* coords_3d, const float* rois, int B, int K, int A, const float* clip_hw, float* out,
                           int32_t* out_counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The KITTI object evaluation (data/kitti_split1/devkit/cpp/evaluate_object*.cpp): precision over 41 recall positions for the
 * image (2D), ground (bird's-eye view) and 3D box of Car / Pedestrian / Cyclist at the three difficulties, and the orientation
 * similarity (AOS), for V variants (MIN_OVERLAP table + optional ground-truth distance cut) in one pass over the data.
 * Rows are float64: det [n_det][14] and gt [n_gt_rows][15], columns below; images are ragged through det_offsets / gt_offsets [I + 1]
 * (int32, ascending from 0); pair_offsets [I + 1] (int64) is the running sum of detections x ground-truth rows per image.
 * Class / type ids: 0 Car, 1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else (a detection: 0..2, else -1).
 * A curve is class * 9 + metric * 3 + difficulty (metric 0 image, 1 ground, 2 3D); a task is variant * 27 + curve.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_KITTI_EVAL_MAX_DET 512   /* detections per image: the assigned_detection bit set of a lane */
#define GNMS_KITTI_EVAL_MAX_GT 1024   /* ground-truth rows per image (DontCare included) */
#define GNMS_KITTI_EVAL_CURVES 27
#define GNMS_KITTI_EVAL_PTS 41
#define GNMS_KITTI_DET_CLASS 0
#define GNMS_KITTI_DET_ALPHA 1
#define GNMS_KITTI_DET_X1 2           /* x1 y1 x2 y2 */
#define GNMS_KITTI_DET_H 6            /* h w l */
#define GNMS_KITTI_DET_T 9            /* t1 t2 t3 (t2: bottom face) */
#define GNMS_KITTI_DET_RY 12
#define GNMS_KITTI_DET_SCORE 13
#define GNMS_KITTI_GT_TYPE 0
#define GNMS_KITTI_GT_TRUNC 1
#define GNMS_KITTI_GT_OCC 2
#define GNMS_KITTI_GT_ALPHA 3
#define GNMS_KITTI_GT_X1 4
#define GNMS_KITTI_GT_H 8
#define GNMS_KITTI_GT_T 11
#define GNMS_KITTI_GT_RY 14
/* Host only, no HIP call: checks the HOST copies of the offsets (ascending from 0, at most GNMS_KITTI_EVAL_MAX_DET detections and
 * GNMS_KITTI_EVAL_MAX_GT ground-truth rows per image -- nothing is truncated, a larger image is an error) and V, and returns the
 * number of (detection, ground truth) pairs. */
int gnms_kitti_eval_plan(const int32_t* det_offsets_host, const int32_t* gt_offsets_host, int I, int V, int64_t* n_pairs);
/* Everything up to the score lists.  min_overlap [V][3 metrics][3 classes], max_depth [V] (+inf: no cut; else `|| gt.t3 > D` joins
 * the ground-truth ignore condition), both on the device.  Outputs: overlaps [3][n_pairs] (metric, then pair_offsets[img] + g * nd + j;
 * criterion -1, on DontCare rows criterion 0), flags [10] ([0] some alpha == -10, [1 + c] eval_image, [4 + c] eval_ground, [7 + c]
 * eval_3d), tp_scores [V * 27][n_gt_rows] (per ground-truth row the score of its true positive, else -inf; rows of curves that are
 * off are not written), n_tp and n_gt [V * 27].  The caller sorts each row of tp_scores in descending order. */
int gnms_kitti_eval_recall(const double* det, const double* gt, const int32_t* det_offsets, const int32_t* gt_offsets,
                           const int64_t* pair_offsets, int I, int n_det, int n_gt_rows, int64_t n_pairs, const double* min_overlap,
                           const double* max_depth, int V, double* overlaps, int32_t* flags, double* tp_scores, int32_t* n_tp,
                           int32_t* n_gt, void* stream);
/* From the sorted score lists to the curves.  Outputs: thresholds [V * 27][41] and n_thresholds [V * 27] (at most 41), counts
 * [V * 27][41][3] = tp fp fn summed over the images, precision [V * 27][41] and aos [V][3 classes][3 difficulties][41] after the
 * max_{i..end} filter, 0 behind n_thresholds and for curves that are off.  similarity [V][9][I][41] is scratch (the per-image
 * orientation similarity, summed in image order).  A threshold with tp + fp = 0 gives the devkit's 0 / 0 = NaN. */
int gnms_kitti_eval_precision(const double* det, const double* gt, const int32_t* det_offsets, const int32_t* gt_offsets,
                              const int64_t* pair_offsets, int I, int n_gt_rows, int64_t n_pairs, const double* min_overlap,
                              const double* max_depth, int V, const double* overlaps, const int32_t* flags, const double* sorted_scores,
                              const int32_t* n_tp, const int32_t* n_gt, double* thresholds, int32_t* n_thresholds, int32_t* counts,
                              double* similarity, double* precision, double* aos, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detections -> the detection rows above, as the devkit would parse them from the reference's result files (lib/train_test.py:102-109,
 * lib/rpn_util.py:1489-1631), appended on the device (csrc/kitti_rows.hip).
 * det [B][Kmax][det_cols = 14] fp32 (x1 y1 x2 y2 score cls u v depth w h l alpha tracker) and counts [B] from gnms_detect3d_assemble,
 * p2_inv [B][4][4] float64.  Per image the first min(nms_topN_post, counts[b]) rows take part; a row is kept when (double)score >
 * score_thres; kept rows keep their order.  Float64 from there: (x, y, z) = rows 0-2 of p2_inv (u depth, v depth, depth, 1), y += h / 2,
 * ry = snap_to_pi(alpha + atan2(-z, x) + pi / 2), alpha = snap_to_pi(ry - atan2(-z, x) - pi / 2); each of the 13 numeric fields v becomes
 * the double that its '%.6f' text parses to (exact for finite |v| < 1e9; other values are stored as they are and counted).
 * class_ids [n_lbls] (1 <= n_lbls <= GNMS_KITTI_ROWS_MAX_LBLS): the row's class id for label index (int)cls - 1; an index outside the
 * table writes class -1 and sets GNMS_KITTI_ROWS_ERR_CLASS.  kept_scratch [B] int32 is scratch.
 * rows [capacity][14] float64 and lbl_index [capacity] int32 (optional: the label index of each row) are appended to behind
 * state[END] rows; offsets [n_offsets] int32 receives the running end at [image_base + b + 1] (the caller keeps offsets[0] = 0).  A row
 * at or beyond `capacity` and an offsets entry at or beyond n_offsets are not stored; state[END] / state[IMAGES] still count them, so
 * the caller sees what was needed.  state [GNMS_KITTI_ROWS_STATE_WORDS] int64, zeroed by the caller before the first call, lives on
 * the device: consecutive calls on one stream append without the host reading anything.  Three stream-ordered launches; no workgroup
 * waits for another. */
#define GNMS_KITTI_ROWS_MAX_LBLS 16
#define GNMS_KITTI_ROWS_STATE_WORDS 8
#define GNMS_KITTI_ROWS_STATE_END 0      /* rows appended so far (needed, not clipped to capacity) */
#define GNMS_KITTI_ROWS_STATE_IMAGES 1   /* images appended so far (needed, not clipped to n_offsets - 1) */
#define GNMS_KITTI_ROWS_STATE_OUTSIDE 2  /* fields that are not finite or not below 1e9 in magnitude */
#define GNMS_KITTI_ROWS_STATE_ERRORS 3   /* GNMS_KITTI_ROWS_ERR_* */
#define GNMS_KITTI_ROWS_STATE_PENDING 4  /* the running end between the write and the commit launch */
#define GNMS_KITTI_ROWS_ERR_CLASS 1      /* a label index outside class_ids */
#define GNMS_KITTI_ROWS_ERR_ANGLE 2      /* an angle so large that 1024 steps of 2 pi did not bring it into (-pi, pi] */
int gnms_kitti_rows_append(const float* det, int det_cols, const int32_t* counts, const double* p2_inv, int B, int Kmax,
                           int nms_topN_post, double score_thres, const int32_t* class_ids, int n_lbls, int32_t* kept_scratch,
                           double* rows, int32_t* lbl_index, int64_t capacity, int32_t* offsets, int n_offsets, int image_base,
                           int64_t* state, void* stream);
/* out[i] = the double that the '%.6f' text of in[i] parses to (in != out); outside_count (optional, device) is incremented for every
 * element that is not finite or not below 1e9 in magnitude (copied as it is). */
int gnms_round6(const double* in, double* out, int64_t n, int64_t* outside_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Between gnms_compute_targets and the NMS block of the training loss: the hard-anchor sampling, the sample weights and the weighted
 * classification term (lib/loss/rpn_3d.py:458-472, 583-612, 885-1001), csrc/sampling.hip, DESIGN.md 3.14.  Stream-ordered launches
 * only, no allocation, no global atomics, no workgroup waits for another: graph-capturable, and the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_SAMPLE_IGN_FLAG 3000     /* labels of ignored anchors (IGN_FLAG, :184) */
#define GNMS_SAMPLE_COUNT_COLS 6      /* n_fg, n_bg, fg_num, bg_num (the reference's quotas, :583-588), sampled fg, sampled bg */
/* target_labels: column 4 of the targets rows, anchor r of image b at target_labels[(b * R + r) * ld_target_labels] (t > 0: foreground
 * of class (int)t, t < 0: background, t == 0: ignore; a class outside [1, C) counts as ignore, a NaN as "label 0, never sampled").
 * prob [B][R][C] (column 0 = background).  skip [B] bytes or NULL: a nonzero byte is an image without a valid ground truth (:406):
 * its labels are 0, nothing of it is sampled, its labels_scores are 0.
 * Quotas per image (:583-588): box_samples = +inf keeps everything; else fg_num = min(round(R box_samples fg_fraction), n_fg) and
 * bg_num = min(round(R box_samples - fg_num), n_bg), round = half to even on float64.  A class is cut to its quota only when
 * 0 < quota != members (:591, :597) -- a quota of 0 keeps the whole class -- and then keeps the anchors with the smallest
 * prob[b][r][label] (NaN last; among equal keys the lower anchor index first).
 * Outputs (all required, every element written): labels [B][R] int64 (0, the class, GNMS_SAMPLE_IGN_FLAG), bbox_weights [B][R]
 * (1 on the sampled foreground), labels_scores [B][R] (prob[b][r][labels] where labels is not the ignore flag), sampled [B][R]
 * bytes (0 no, 1 foreground, 2 background), fg_index [B][R] int32: the sampled foreground in ascending anchor order, -1 behind
 * fg_counts[b] (gnms_select_topk's candidates / candidate_counts), counts [B][GNMS_SAMPLE_COUNT_COLS] int32.
 * workspace: gnms_sample_anchors_workspace_bytes(B, R) bytes, 16-byte aligned, every byte written before it is read. */
size_t gnms_sample_anchors_workspace_bytes(int B, int R);
int gnms_sample_anchors(const float* target_labels, int64_t ld_target_labels, const float* prob, const uint8_t* skip, int B, int R,
                        int C, double box_samples, int has_fg_fraction, double fg_fraction, int64_t* labels, float* bbox_weights,
                        float* labels_scores, uint8_t* sampled, int32_t* fg_index, int32_t* fg_counts, int32_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream);
/* :913-1001 from gnms_sample_anchors' outputs and the logits cls [B][R][C].  Weights (:913-961): 1 on every sampled anchor, the
 * foreground (has_fg_fraction and a sampled foreground in the batch) (f / (1 - f)) * (sampled bg / sampled fg) over the batch;
 * focal_loss != 0: times (1 - labels_scores) ** focal_loss; all in float64, rounded once into labels_weight [B][R].
 * Term (:976-1001): over the anchors with labels_weight > 0, cross entropy of the float32 log-softmax times the weight, clamped to
 * [0, 2000], summed in float64, mean rounded to float32, times cls_2d_lambda -> loss [1] (0 without an active anchor or with
 * cls_2d_lambda == 0).  dcls [B][R][C] = dloss / dcls (0 on inactive anchors and where the weighted loss left the clamp).
 * acc [2] float64 = accuracy of argmax(cls) over all foreground-labelled anchors / all anchors labelled 0 (:893-907; NaN when there
 * is none); stat_counts [5] int32 = fg correct, fg all, bg correct, bg all, active anchors.
 * workspace: gnms_cls_loss_workspace_bytes(B, R) bytes, 8-byte aligned. */
size_t gnms_cls_loss_workspace_bytes(int B, int R);
int gnms_cls_loss(const float* cls, const int64_t* labels, const float* labels_scores, const uint8_t* sampled, const int32_t* counts,
                  int B, int R, int C, int has_fg_fraction, double fg_fraction, double focal_loss, double cls_2d_lambda,
                  float* labels_weight, float* loss, float* dcls, double* acc, int32_t* stat_counts, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * What the training loss does with the sampled foreground (lib/loss/rpn_3d.py:1154-1407, fed by :206-233, :316-363, :477-579,
 * :617-621): the 2D and 3D smooth-L1 terms, the axis / head cross entropies, the -log IoU term, the acceptance weighting, the
 * uncertainty term with its running weight, the statistics and the gradients of the heads.  csrc/regression.hip, DESIGN.md 3.15.
 * Configuration: decomp_alpha, orientation_bins = 0, infer_2d_from_3d = has_un = weigh_3D_regression_loss_by_gt_iou3d = False.
 * Two stream-ordered launches, no allocation, no global atomics, no workgroup waits for another, nothing read back:
 * graph-capturable with gnms_sample_anchors and gnms_cls_loss, and the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_REG_STATS 14          /* stats: bbox_2d, bbox_3d, un, iou_2d_los, cen, cen_dist_lt_0.2, z, rot, iou_2d, axis, head, conf,
                                      total, the uncertainty weight in use */
#define GNMS_REG_STAT_COUNTS 24    /* stat_counts: active anchors; finite elements of x, y, z, w, h, l, rot, axis, head before the
                                      weighting [1..9]; of x .. rot as the term uses them [10..16]; finite IoUs, IoUs != 0, finite
                                      -log IoU [17..19]; weighted, the IoU term exists [20..21]; 0 */
/* Active anchors of image b: fg_index[b][0 .. fg_counts[b]) of gnms_sample_anchors (an entry outside [0, R) is passed over); counts
 * [B][GNMS_SAMPLE_COUNT_COLS]: only images with counts[b][2] > 0 (the quota fg_num, :617) get an IoU, the others' IoUs are 0.
 * Heads: bbox_2d [B][R][4]; bbox_3d [B][R][ld_bbox_3d >= 10] (x, y, z, w, h, l, rsin, rcos, axis, head; axis and head in [0, 1]);
 * acceptance [B][R] or NULL.  Rows read where they lie, anchor r of image b at (b * R + r) * ld: transforms (>= 14 columns, normalised),
 * raw_gt (>= 21), rois (>= 4), rois_3d (>= 11); rois_3d_cen [B][R][2]; p2 [B][p2_rows = 3 or 4][4] and scale_factor [B], float64, on
 * the device.  means / stds: 13 values each ON THE HOST, read before the call returns.
 * Terms (all means over the B images' active anchors together; per-anchor arithmetic in float64):
 *   2D (:1163-1191)   bbox_2d_lambda * sum_k mean smooth_l1(bbox_2d[k] - transforms[k]); the prediction as the network gave it (the
 *                     reference's has been denormalised in place by bbox_transform_inv; equal for means 0, stds 1)
 *   3D (:1211-1373)   smooth-L1 of bbox_3d[0..5] against transforms[5..10], of rsin against transforms[12] where raw_gt[19] == 1, else
 *                     of rcos against transforms[13]; binary cross entropy of axis / head against raw_gt[19] / raw_gt[20].  With
 *                     bbox_un_dynamic, init = (sum of the seven means over finite elements) * bbox_3d_lambda + (the two cross
 *                     entropies' means over finite elements) * bbox_axis_head_lambda before any weighting, and un_state = {n_frames,
 *                     weight} (float64, on the device) is updated: n_frames 0 -> weight = init, n_frames = 1; else n_frames =
 *                     min(100, n_frames + 1), weight = init / n_frames + weight * (n_frames - 1) / n_frames.  Every term is then
 *                     multiplied by acceptance when use_acceptance, or when bbox_un_dynamic and the new weight > 0 (decided on the
 *                     device).  Term = (sum of the seven means over finite elements + (plain means of the cross entropies) *
 *                     bbox_axis_head_lambda) * bbox_3d_lambda.
 *   un (:1375-1382)   weight > 0 (bbox_un_dynamic: un_state's, else bbox_un_lambda): mean(1 - acceptance) * weight
 *   IoU (:1390-1405)  iou_2d_lambda != 0 and some active IoU != 0: iou_2d_lambda * mean over finite elements of -log IoU; IoU of
 *                     core.py:522-529 (no + 1) between bbox_transform_inv of bbox_2d and of transforms[0..3], both from rois[b]
 * Outputs, every element written: loss [1]; stats [GNMS_REG_STATS] float64; stat_counts [GNMS_REG_STAT_COUNTS]; d_bbox_2d,
 * d_bbox_3d (rows of ld_bbox_3d), d_acceptance (with acceptance) = d loss / d head, 0 off the active set, in unread columns and on an
 * element that an isfinite filter dropped.  No active anchor: loss 0, gradients 0, stats[0..12] NaN, un_state untouched.
 * workspace: gnms_reg_loss_workspace_bytes(B, R) bytes, 8-byte aligned; d_bbox_2d 16-byte aligned. */
size_t gnms_reg_loss_workspace_bytes(int B, int R);
int gnms_reg_loss(const float* bbox_2d, const float* bbox_3d, int ld_bbox_3d, const float* acceptance, const float* transforms,
                  int64_t ld_transforms, const float* raw_gt, int64_t ld_raw_gt, const float* rois, int ld_rois, const float* rois_3d,
                  int ld_rois_3d, const float* rois_3d_cen, const double* p2, int p2_rows, const double* scale_factor,
                  const int32_t* fg_index, const int32_t* fg_counts, const int32_t* counts, int B, int R, const double* means,
                  const double* stds, double bbox_2d_lambda, double bbox_3d_lambda, double bbox_axis_head_lambda, double iou_2d_lambda,
                  int use_acceptance, double bbox_un_lambda, int bbox_un_dynamic, double* un_state, float* loss, double* stats,
                  int32_t* stat_counts, float* d_bbox_2d, float* d_bbox_3d, float* d_acceptance, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The after-NMS block of the loss (lib/loss/rpn_3d.py:721-825, :1091-1148) from the heads (csrc/after_nms.hip), around
 * gnms_select_topk, the layer and gnms_best_targets.  Stream-ordered launches only, no allocation, nothing read back.
 * ------------------------------------------------------------------------------------------------ */
/* gnms_aploss with an implicit tail: image b is ranked as if tail_counts[b] further negatives of logit 0 followed its explicit boxes
 * (the sampled foreground beyond the boxes that went through the NMS, :1124-1128, whose scores_after_nms and targets_after_nms are 0).
 * Where 0 >= min positive - 1 (aploss.py:32-35) every positive's b_p gets tail * clamp((0 - x_p) / 2 + 0.5, 0, 1); the tail has no
 * gradient output.  One workgroup per image in LDS whatever B is: N <= 4096, GNMS_ERR_UNSUPPORTED above.  tail_counts all 0: the bits
 * of gnms_aploss's LDS route. */
int gnms_aploss_tail(const float* logits, const float* targets, int B, int N, const int32_t* counts, const int32_t* tail_counts,
                     float positive_label, float negative_label, float* loss, float* grad, void* stream);
/* Gather and decode of the selected anchors, one launch.  sel_index [B][K] / sel_counts [B] from gnms_select_topk.  Heads bbox_2d
 * [B][R][4] (16-byte aligned), bbox_3d [B][R][D3 >= 10]; raw_gt (>= 21 columns: [19] axis label, [20] head label), rois (>= 4), rois_3d
 * (>= 11) read where they lie, anchor r of image b at (b * R + r) * ld; rois_3d_cen [B][R][2]; p2 [B][p2_rows][4] and scale_factor [B]
 * float64 on the device; means / stds 13 values each ON THE HOST.  gts_val [B][M][4], gts_3d [B][M][ld_gts_3d >= 11] float64 and
 * val_counts [B] as gnms_compute_targets takes them.
 * boxes2d [B][K][4] = bbox_transform_inv(rois[b], bbox_2d, means[:4], stds[:4]) of the selected rows (the device code of
 * gnms_bbox_transform_inv; not divided by the scale).  cuboids [B][K][7] = x y z w h l ry in camera space, fp32 in the reference's
 * operation order (:318-363, :532-574): the rotation is rois_3d[9] + rsin where raw_gt[19] == 1, else rois_3d[10] + rcos, + pi where
 * raw_gt[20] == 1, snapped into (-pi, pi] (bounded loop; a non-finite angle stays), then alpha -> rotation_y (util.py:635-638).
 * gt_params [B][M][7] = gts_3d columns 7 8 9 3 4 5 10, gt_boxes [B][M][4] (:801-811).  Rows behind an image's count are zero. */
int gnms_after_nms_decode(const int64_t* sel_index, const int32_t* sel_counts, int B, int K, int R, const float* bbox_2d,
                          const float* bbox_3d, int D3, const float* raw_gt, int64_t ld_raw_gt, const float* rois, int ld_rois,
                          const float* rois_3d, int ld_rois_3d, const float* rois_3d_cen, const double* p2, int p2_rows,
                          const double* scale_factor, const double* means_host, const double* stds_host, const double* gts_val,
                          const double* gts_3d, int ld_gts_3d, int M, const int32_t* val_counts, float* boxes2d, float* cuboids,
                          float* gt_params, float* gt_boxes, void* stream);
/* One workgroup.  mode 0: rank per image, 1: rank all images at once, 2: classify.  fg_counts [B] = sampled foreground per image.
 * phase 0 (in front of gnms_aploss_tail): tail_counts [B + 1] = max(fg_counts - sel_counts, 0) per image, then their sum;
 *   targets [B][K] (written) = 1 where some best_index[b][m] (gnms_best_targets, [B][M]) names the box, else 0;
 *   targets_padded [B][K] = targets, -1 behind sel_counts (mode 1 ranks it as ONE row of B * K with the summed tail).
 * phase 1: img_cnt [1] = #{b: fg_counts[b] > 0}; loss [2 + B] = the loss, the statistic (the same value), the per-image AP losses
 *   (0 in modes 1, 2); dprob [B][K] = d loss / d (rescored probability), 0 behind sel_counts.
 *   mode 0: loss = lambda * sum over counted images of ap_loss[b] / img_cnt, dprob = ap_grad * lambda / img_cnt (:1121-1131);
 *   mode 1: loss = lambda * ap_loss[0] (:1119); no sampled foreground in the batch: loss 0, dprob 0 (:1100-1101).
 *   mode 2 (:1103-1115): binary cross entropy of prob against targets, logs clamped at -100, negatives weighted by
 *   (n_pos / n_neg)^0.25 when both are positive, mean over the finite elements; the zero tail counts in n_neg and in the mean; an
 *   element the filter drops gets gradient 0. */
int gnms_after_nms_finish(int phase, int mode, int B, int K, const int32_t* fg_counts, const int32_t* sel_counts, const float* prob,
                          float* targets, const float* ap_loss, const float* ap_grad, float after_nms_lambda,
                          int32_t* tail_counts, float* targets_padded, float* loss, int32_t* img_cnt, float* dprob,
                          const int64_t* best_index, int M, void* stream);
/* The backward scatter: dscore [B][K] = d loss / d (score that went into the layer) -> the heads' dense gradients, every element
 * written, 0 off the selection.  acceptance [B][R] with dacceptance, prob [B][R][C] with cls_pred [B][R] (gnms_detect3d_scores) and
 * dprob where the scores read max(prob[1:]): dacceptance = dscore (* that maximum), dprob[cls_pred] = dscore (* acceptance). */
int gnms_after_nms_scatter(const int64_t* sel_index, const int32_t* sel_counts, const float* dscore, int B, int K, int R, int C,
                           const float* acceptance, const float* prob, const int32_t* cls_pred, float* dacceptance, float* dprob,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * The RPN heads' maps -> the five tensors every entry behind the network reads (csrc/heads.hip): what
 * models/densenet121_3d_dilate_decomp_alpha.py:166-215 builds from its fifteen 1x1 convolutions.  One launch each, no workspace, no
 * atomics, nothing filled beforehand, nothing read back; the host arrays are read before the call returns and travel in the kernel's
 * arguments, so both entries can be captured into a graph.
 * R = A * H * W, anchor row r = (a * H + h) * W + w (locate_anchors(..., convert_tensor=True); view(B, C, A * H, W) + flatten_tensor).
 * maps [15], float32 on the device: the class logits [B][C * A][H][W] (channel c * A + a), the thirteen box maps [B][A][H][W] in the
 * order x y w h x3d y3d z3d w3d h3d l3d alpha axis head (axis and head before their sigmoid), the acceptance map [B][A][H][W] or NULL.
 * Image b of map k starts batch_strides[k] elements behind image b - 1 (>= 0; a channel slice of a stacked output keeps the stacked
 * stride); its [., H, W] block is contiguous.
 *   cls [B][R][C]      = cls_map[b].flat[c * R + r]
 *   prob [B][R][C]     = softmax over c: exp(x - max) / sum, expf and a true division
 *   bbox_2d [B][R][4]  = x y w h
 *   bbox_3d [B][R][10] = x3d y3d z3d w3d h3d l3d alpha alpha sigmoid(axis) sigmoid(head), sigmoid(x) = 1 / (1 + expf(-x))
 *   acceptance [B][R]  = sigmoid(acceptance map); not touched without the map
 * cls, prob, bbox_2d, bbox_3d 16-byte aligned.  2 <= C <= 16 (GNMS_ERR_UNSUPPORTED outside).  B = 0: GNMS_OK, nothing is done. */
int gnms_heads_assemble(const void* const* maps, const long long* batch_strides, int B, int A, int H, int W, int C, float* cls,
                        float* prob, float* bbox_2d, float* bbox_3d, float* acceptance, void* stream);
/* The backward: prob, bbox_3d, acceptance as gnms_heads_assemble wrote them, the five cotangents (contiguous rows; one that is NULL is
 * zero and then needs no forward tensor either), and grad_maps [15]: contiguous float32 [B][.][H][W] like the maps, every element
 * written; an entry that is NULL is not computed.
 *   d cls_map[c] = g_cls[c] + prob[c] * (g_prob[c] - sum_j g_prob[j] * prob[j])
 *   d alpha = g_bbox_3d[6] + g_bbox_3d[7];  d axis = g_bbox_3d[8] * s * (1 - s) with s = bbox_3d[8], head ([9]) and acceptance alike;
 *   the other ten maps get their cotangent column.
 * prob and the cotangents of cls, prob, bbox_2d, bbox_3d 16-byte aligned, bbox_3d 8-byte. */
int gnms_heads_assemble_backward(const float* prob, const float* bbox_3d, const float* acceptance, const float* g_cls,
                                 const float* g_prob, const float* g_bbox_2d, const float* g_bbox_3d, const float* g_acceptance, int B,
                                 int A, int H, int W, int C, void* const* grad_maps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RPN_3D_loss around its terms (csrc/loss.hip): the ground truths of a batch from packed records, the total with the
 * reference's statistics, and the whole backward.  One launch each, no workspace, no atomics, nothing filled beforehand, nothing read
 * back: graph-capturable with the terms' entries between them.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_LOSS_RECORD_COLS 24   /* a ground truth: bbox_full x y w h [0..3], bbox_3d [4..19], class id [20] (1 + index in lbls, 0 for a
                                      class of ilbls, -1 for neither), ign [21] (0 / not 0), visibility [22], trunc [23] */
#define GNMS_LOSS_MAX_GTS 256      /* records per image (GNMS_TARGETS_MAX_GTS) */
#define GNMS_LOSS_STATS 18         /* stats: fg, bg, cls, the after-NMS statistic, bbox_2d, cen, cen_dist_lt_0.2, axis, head, conf, bbox_3d,
                                      un, z, rot, iou_2d, iou_2d_los, total (the order of the reference's list), the uncertainty weight */
/* lib/loss/rpn_3d.py:399-419.  records [B][capacity][GNMS_LOSS_RECORD_COLS] float64, counts [B] (clamped to 0..capacity), in the order
 * the reference iterates the ground truths.  Per record, determine_ignores (rpn_util.py:937-962) as the loss calls it, in float64:
 * ign = ign | visibility < min_gt_vis | h < min_gt_h | h > max_gt_h (scale_factor 1; the loss leaves max_gt_h at 10e10) | class id == 0
 * (| trunc > max(1 - min_gt_vis, 0) with use_trunc); rmv = class id < 0.  bbXYWH2Coords: x2 = w + (x - 1), y2 = h + (y - 1).
 * Outputs, every element written, rows in input order: gts_val [B][capacity][4] / box_lbls [B][capacity] (the class id) / gts_3d
 * [B][capacity][16] of the records with !rmv & !ign, gts_ign [B][capacity][4] of those with !rmv & ign, val_counts / ign_counts [B];
 * rows behind a count are zero.  One workgroup per image; 1 <= capacity <= GNMS_LOSS_MAX_GTS (GNMS_ERR_UNSUPPORTED outside).
 * records, gts_val, gts_3d, gts_ign 16-byte aligned. */
int gnms_gt_filter(const double* records, const int32_t* counts, int B, int capacity, double min_gt_vis, double min_gt_h,
                   double max_gt_h, int use_trunc, double* gts_val, int32_t* box_lbls, double* gts_3d, double* gts_ign,
                   int32_t* val_counts, int32_t* ign_counts, void* stream);
/* cls_loss [1] / cls_acc [2] of gnms_cls_loss, after_loss = the loss array of gnms_after_nms_finish (phase 1), reg_stats
 * [GNMS_REG_STATS] / reg_counts [GNMS_REG_STAT_COUNTS] of gnms_reg_loss; a term that is NULL is absent.
 * total [1] = ((((((0 + cls) + after) + bbox_2d) + bbox_3d) + un) + iou_2d_los) in fp32, the reference's order of `loss +=` (:999,
 * :1138, :1190, :1371, :1380, :1403), each regression term rounded to fp32 once; the regression terms only with an active anchor
 * (reg_counts[0] > 0, :1154).  stats [GNMS_LOSS_STATS] float64, every element written (0 for an absent term; the regression
 * statistics are NaN without an active anchor, as gnms_reg_loss reports them). */
int gnms_loss_combine(const float* cls_loss, const double* cls_acc, const float* after_loss, const double* reg_stats,
                      const int32_t* reg_counts, float* total, double* stats, void* stream);
/* The backward of the whole loss.  upstream [1]: d L / d total on the device.  The terms' dense gradients over rows = B * R anchors:
 * dcls [rows][C] (gnms_cls_loss), dprob [rows][C] and dacc [rows] (gnms_after_nms_scatter), d2 [rows][4], d3 [rows][D3], da [rows]
 * (gnms_reg_loss; d3 is zero in the columns the loss does not read); one that is NULL is zero.
 *   g_cls = upstream * dcls, g_prob = upstream * dprob, g_bbox_2d = upstream * d2, g_bbox_3d = upstream * d3,
 *   g_acceptance = upstream * (da + dacc)
 * An output that is NULL is not computed; every element of the others is written (zeros where the inputs are NULL).  All buffers
 * contiguous float32, 16-byte aligned. */
int gnms_loss_grad_combine(const float* upstream, long long rows, int C, int D3, const float* dcls, const float* dprob, const float* d2,
                           const float* d3, const float* da, const float* dacc, float* g_cls, float* g_prob, float* g_bbox_2d,
                           float* g_bbox_3d, float* g_acceptance, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The data-set reduction of compute_bbox_stats (lib/rpn_util.py:547-736; csrc/bbox_stats.hip): from the raw
 * (un-normalised) transforms of gnms_compute_targets to bbox_means / bbox_stds.  One launch each, no workspace, no atomics, nothing
 * filled beforehand, nothing read back.  Every addition happens in an order the inputs alone fix: the results do not depend on the
 * batch size, on the order the batches come in, or on the run.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_BBOX_STATS_COLS 13    /* the statistics columns: transforms[:, 0:4] and transforms[:, 5:14] (decomp_alpha) */
/* transforms [B][R][ld] float32, ld >= 14; image b of the batch is image image_ids[b] (device int32) of a data set of n_images, and
 * its partials go to that position (an id outside 0..n_images-1: the image writes nothing).  Foreground = transforms[:, 4] > 0
 * (:629), taken in row order.  counts [n_images] int32: the image's foreground count (both passes).
 * means NULL, the mean pass: sums [n_images][GNMS_BBOX_STATS_COLS] float32 = np.sum(transforms[fg, cols], axis=0) bit for bit (from
 * +0, one float32 addition per foreground row in row order; 0 without foreground).
 * means [GNMS_BBOX_STATS_COLS] float64 on the device, the deviation pass: sq_sums [n_images][GNMS_BBOX_STATS_COLS] float64 = the sum
 * of (double(x) - mean)^2 in row order.  The other pass's array may be NULL.  One workgroup per image.  B = 0: GNMS_OK, nothing is
 * done; B > n_images or ld < 14: GNMS_ERR_INVALID_ARGUMENT. */
int gnms_bbox_stats_partials(const float* transforms, int B, int R, int64_t ld, const int32_t* image_ids, int n_images,
                             const double* means, float* sums, double* sq_sums, int32_t* counts, void* stream);
/* The partials of the images with used[i] != 0 (uint8 [n_images]; the others, the images without ground truths of :587, are never
 * read) and counts[i] > 0, added in image order in double-double, the counts in int64.
 * deviation = 0: count[0] = the total foreground count; out [GNMS_BBOX_STATS_COLS] = sums / (count + 1e-10) (:579, :652).
 * deviation = 1: reads count[0] (the mean pass's, :721) and sq_sums; out = sqrt(sq_sums / (count + 1e-10)).
 * Quotient and root are evaluated in double-double and rounded to float64 once.  Every element of out is written. */
int gnms_bbox_stats_finish(int deviation, const uint8_t* used, int n_images, const float* sums, const double* sq_sums,
                           const int32_t* counts, long long* count, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The image front end of lib/augmentations.py (Augmentation / Preprocess and the RGB swap + transpose that follow them;
 * csrc/preprocess.hip): one launch per batch, no workspace, no atomics.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_PREPROCESS_DESC 5     /* int64 per image: byte offset into src, H, W, width after the resize (before crop / pad), mirror */
/* src: src_bytes of uint8 on the device holding B images, HWC, 3 channels, BGR, each at its descriptor's offset; table [B][5] int64 on
 * the device; means / stds: 3 floats each ON THE HOST, in the order the reference applies them (entry 0 -> blue), read before the
 * call returns.  out [B][3][H_out][W_out] float32, RGB planes, 16-byte aligned.  Per output pixel: the source column mirrored when
 * the flag is set, bilinear taps at (d + 0.5) * (src / dst) - 0.5 (double, rounded to float; floor + fraction, both taps clamped to
 * the edge; horizontal pass then vertical pass in float32), columns >= the resized width are 0 before the normalisation, then
 * x / 255, - mean, / std in float32.  H_out is the height after the resize.  Only magnification is meant (src / dst <= 1); the entry
 * does not check it, the Python wrapper does.  An image whose descriptor does not lie inside src (or with H, W outside 1..2^20) is
 * not read and its output is not written.  B = 0: GNMS_OK, nothing is done. */
int gnms_preprocess_images(const uint8_t* src, int64_t src_bytes, const int64_t* table, int B, int H_out, int W_out,
                           const float* means, const float* stds, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The optimiser step of lib/core.py:99-113 (clip_grad_value_, torch.optim.SGD.step with momentum and weight decay, zero_grad;
 * csrc/optim.hip): one launch per parameter group, no workspace, no float atomics, nothing read on the host.
 * ------------------------------------------------------------------------------------------------ */
#define GNMS_SGD_ROW 4             /* int64 per row of either table */
/* tensors [n_tensors][4] int64 on the device: the addresses of p, g and buf (float32, contiguous, numel elements each) and numel.
 * tasks [n_tasks][4] int64 on the device: tensor, start, count, kind; elements start .. start + count - 1 of that tensor.  kind 1: p, g
 * and buf are 16-byte aligned at `start` (16 bytes per lane, the last count % 4 elements one by one; a task whose addresses are not is
 * done one by one all the same); kind 0: one by one.  A task that does not lie inside its tensor is skipped.  Every element must lie in
 * exactly one task.  Per element, in float32, each operation rounded on its own:
 *     g' = g < -c ? -c : (g > c ? c : g)   (use_clip != 0; NaN stays NaN)      d = g' + f32(weight_decay) * p
 *     buf = f32(momentum) * buf + d          p = p + f32(-lr) * buf              g = 0
 * loss: NULL, or a float32 scalar on the device: unless *loss > 0 (so also for NaN) p and buf are left as they are and g is zeroed.
 * lr_table: NULL (lr is the argument), or lr_table_len float64 on the device: lr = lr_table[min(max(state[0], 0), lr_table_len - 1)].
 * state: int64 [2] on the device, {iteration, 0}.  advance != 0: the launch adds 1 to state[0] after every workgroup has read it
 * (state[1] is the ticket they take, 0 again when the launch ends).  grid: workgroups, 0 = four per compute unit; nt: bit 0 = the 16-byte
 * loads non-temporal, bit 1 = the 16-byte stores (0..3; the same values either way).  n_tasks = 0: only the counter moves. */
int gnms_sgd_step(const int64_t* tensors, int n_tensors, const int64_t* tasks, int n_tasks, double lr, double momentum,
                  double weight_decay, double clip_value, int use_clip, const float* loss, const double* lr_table, int lr_table_len,
                  int64_t* state, int advance, int grid, int nt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GROOMED_NMS_HIP_H */
