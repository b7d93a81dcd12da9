"""The after-NMS block of the RPN loss from the heads, on the GPU (csrc/after_nms.hip): what lib/loss/rpn_3d.py does
under use_nms_in_loss, on top of targets.compute_targets_batched and sampling.sample_anchors.

  after_nms_loss   :721-737 (scores, the at most max_nms_boxes best sampled foreground anchors per image), :316-363 + :532-574 (their
                   2D boxes and camera-space cuboids, decoded for the selected anchors only), :746-793 (GrooMeD-NMS on their 2D
                   overlaps), :801-825 (the best box per ground truth), :1091-1148 (the AP or cross-entropy term over every sampled
                   foreground anchor) and the gradient back into the acceptance head (and prob where the scores read it)
The chain is gnms_detect3d_scores (only where the class confidence takes part) -> gnms_select_topk -> gnms_after_nms_decode
(-> gnms_project_boxes3d) -> the layer -> gnms_best_targets -> gnms_after_nms_finish -> gnms_aploss_tail -> gnms_after_nms_finish ->
the layer's backward -> gnms_after_nms_scatter.  Device tensors in, device tensors out; nothing is read back and every launch is
stream-ordered, so the call can be captured in a graph behind sample_anchors.  There is no CPU implementation here.

Deliberate differences from the reference:
  * the sampled foreground beyond the selected boxes is not materialised: the reference ranks it as explicit zeros (:1124-1128), here
    the AP kernel adds its closed-form contribution to every positive's rank (gnms_aploss_tail).  The value is the same.
  * the AP loss sees an image's boxes in selection order (descending score), the reference in anchor order; only the order of the
    fp32 additions differs.
  * mode "classify": an element that the isfinite filter drops (:1115) gets gradient 0; the reference's backward yields NaN there.
  * ties among equal scores at the cut go to the lower anchor index (torch.sort leaves them undefined).
"""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .regression import _rows

__all__ = ["after_nms_loss", "STAT_NAME"]

STAT_NAME = {"rank": "bbox_after_nms_rank", "classify": "bbox_after_nms_class"}
_PRUNE = ("linear", "sigmoidal", "soft_nms")


class _AfterNMSLoss(torch.autograd.Function):
    """loss = the finish kernel's scalar; its gradients w.r.t. the heads were written by the same call and are only scaled here"""

    @staticmethod
    def forward(ctx, run, acceptance, prob):
        loss, dacc, dprob = run()
        empty = loss.new_empty(0)
        ctx.save_for_backward(dacc if dacc is not None else empty, dprob if dprob is not None else empty)
        ctx.like = [(t.dtype, t.shape) if (t is not None and g is not None) else None for t, g in ((acceptance, dacc), (prob, dprob))]
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grads = []
        for g, like in zip(ctx.saved_tensors, ctx.like):
            grads.append((g * grad_output).to(like[0]).reshape(like[1]) if like is not None else None)
        return (None,) + tuple(grads)


def _after_nms_term(prob, acceptance, bbox_2d, bbox_3d, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, gts_val, gts_3d,
                    val_counts, *, means, stds, after_nms_lambda=0.05, after_nms_loss_mode="rank", rank_boxes_of_all_images_at_once=False,
                    rank_with_class_confidence=False, best_target_box_beta=0.3, nms_threshold=0.4, pruning_method="linear", temperature=0.1,
                    valid_box_prob_threshold=0.3, group_boxes=True, mask_group_boxes=True, group_size=100, diff_nms_boxes_2d="normal",
                    overlap_in_nms="2d", max_nms_boxes=500, decomp_alpha=True):
    """after_nms_loss up to the launches -> (run, info, use_prob): run() launches the chain on the detached heads and returns (loss [],
    dacc [B, R] or None, dprob [B, R, C] or None), loss being element 0 of gnms_after_nms_finish's loss array; info is filled by it;
    use_prob: the scores read prob.  (Shared with loss.RPN_3D_loss, which scales the gradients in its one backward launch.)"""
    if after_nms_loss_mode not in ("rank", "classify"):
        raise NotImplementedError("after_nms_loss implements after_nms_loss_mode 'rank' and 'classify', not %r" % (after_nms_loss_mode,))
    if overlap_in_nms != "2d":
        raise NotImplementedError("after_nms_loss implements overlap_in_nms='2d', not %r" % (overlap_in_nms,))
    if not decomp_alpha:
        raise NotImplementedError("after_nms_loss implements decomp_alpha=True")
    if diff_nms_boxes_2d not in ("normal", "projected"):
        raise ValueError("diff_nms_boxes_2d is 'normal' or 'projected', got %r" % (diff_nms_boxes_2d,))
    if pruning_method not in _PRUNE:
        raise NotImplementedError("Pruning method not implemented!")
    if acceptance is None and prob is None:
        raise ValueError("the scores need `acceptance` or `prob`")
    use_prob = acceptance is None or bool(rank_with_class_confidence)
    mode = 2 if after_nms_loss_mode == "classify" else (1 if rank_boxes_of_all_images_at_once else 0)
    K = int(max_nms_boxes)
    if K < 1:
        raise ValueError("max_nms_boxes must be >= 1, got %d" % K)
    means = [float(v) for v in means]
    stds = [float(v) for v in stds]
    if len(means) < 13 or len(stds) < 13:
        raise ValueError("means and stds hold 13 values each, got %d and %d" % (len(means), len(stds)))
    if not isinstance(bbox_2d, torch.Tensor) or bbox_2d.dim() != 3 or bbox_2d.shape[2] != 4:
        raise ValueError("bbox_2d must be [B, R, 4]")
    B, R = int(bbox_2d.shape[0]), int(bbox_2d.shape[1])
    if not isinstance(bbox_3d, torch.Tensor) or bbox_3d.dim() != 3 or tuple(bbox_3d.shape[:2]) != (B, R) or bbox_3d.shape[2] < 10:
        raise ValueError("bbox_3d must be [B, R, >= 10] = [%d, %d, >= 10]" % (B, R))
    if acceptance is not None and tuple(acceptance.shape) != (B, R):
        raise ValueError("acceptance must be [B, R] = [%d, %d], got %s" % (B, R, tuple(acceptance.shape)))
    if use_prob and (not isinstance(prob, torch.Tensor) or prob.dim() != 3 or tuple(prob.shape[:2]) != (B, R) or prob.shape[2] < 2):
        raise ValueError("prob must be [B, R, >= 2] = [%d, %d, >= 2]" % (B, R))
    if tuple(sample.fg_index.shape) != (B, R) or sample.fg_counts.numel() != B or tuple(sample.counts.shape) != (B, 6):
        raise ValueError("sample does not belong to heads of [B, R] = [%d, %d]" % (B, R))
    if any(t.dtype != torch.int32 or not t.is_contiguous() for t in (sample.fg_index, sample.fg_counts, sample.counts)):
        raise ValueError("sample.fg_index, fg_counts and counts must be contiguous int32 tensors (sample_anchors' outputs)")
    if mode == 1 and B * K > 4096:
        raise ValueError("rank_boxes_of_all_images_at_once ranks B * max_nms_boxes <= 4096 boxes in one workgroup, got %d" % (B * K))
    if K > 4096:
        raise ValueError("max_nms_boxes <= 4096, got %d" % K)
    raw_gt = targets.raw_gt if hasattr(targets, "raw_gt") else targets[1]
    dev = sample.fg_index.device
    raw_gt, ld_gt = _rows(raw_gt, dev, B, R, 21, "targets.raw_gt")
    rois, ld_rois = _rows(rois, dev, B, R, 4, "rois")
    rois_3d, ld_r3 = _rows(rois_3d, dev, B, R, 11, "rois_3d")
    cen, _ = _rows(rois_3d_cen, dev, B, R, 2, "rois_3d_cen")
    cen = cen[:, :, :2].contiguous()
    p2 = torch.as_tensor(p2).to(device=dev, dtype=torch.float64).contiguous()
    if p2.dim() != 3 or p2.shape[0] != B or p2.shape[1] not in (3, 4) or p2.shape[2] != 4:
        raise ValueError("p2 must be [B, 3 or 4, 4], got %s" % (tuple(p2.shape),))
    scale = torch.as_tensor(scale_factor).to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    if scale.numel() != B:
        raise ValueError("scale_factor must be [B] = [%d]" % B)
    gv = torch.as_tensor(gts_val).to(device=dev, dtype=torch.float64)
    g3 = torch.as_tensor(gts_3d).to(device=dev, dtype=torch.float64)
    if gv.dim() != 3 or gv.shape[0] != B or gv.shape[2] != 4 or g3.dim() != 3 or tuple(g3.shape[:2]) != tuple(gv.shape[:2]) or g3.shape[2] < 11:
        raise ValueError("gts_val must be [B, M, 4] and gts_3d [B, M, >= 11], got %s and %s" % (tuple(gv.shape), tuple(g3.shape)))
    vc = torch.as_tensor(val_counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if vc.numel() != B:
        raise ValueError("val_counts must be [B] = [%d]" % B)
    if gv.shape[1] == 0:                                  # no ground truth anywhere: one zero row that no count reaches
        gv, g3 = gv.new_zeros((B, 1, 4)), g3.new_zeros((B, 1, 11))
    gv, g3 = gv.contiguous(), g3.contiguous()
    M, ld_g3 = int(gv.shape[1]), int(g3.shape[2])
    if not dev.type == "cuda" or any(t.device != dev for t in (sample.fg_counts, sample.counts)):
        raise ValueError("sample must lie on one GPU (got %s); there is no CPU fallback" % dev)
    lib = _lib.load()
    from . import groomed_nms as G
    from . import proposals
    D3 = int(bbox_3d.shape[2])
    C = int(prob.shape[2]) if use_prob else 0
    c_means = (ctypes.c_double * 13)(*means[:13])
    c_stds = (ctypes.c_double * 13)(*stds[:13])
    f32 = dict(dtype=torch.float32, device=dev)
    info = {}

    def run():
        st = stream_ptr(dev)
        x2 = bbox_2d.detach().to(**f32).contiguous()
        x3 = bbox_3d.detach().to(**f32).contiguous()
        xa = acceptance.detach().to(**f32).contiguous() if acceptance is not None else None
        xp = prob.detach().to(**f32).contiguous() if use_prob else None
        cls_pred = None
        with _lib.on_device(dev):
            if use_prob:                                  # :722-727
                scores = torch.empty((B, R), **f32)
                cls_pred = torch.empty((B, R), dtype=torch.int32, device=dev)
                check(lib.gnms_detect3d_scores(ptr(xp), ptr(xa), 1, B, R, C, ptr(scores), ptr(cls_pred), st), "gnms_detect3d_scores")
            else:
                scores = xa
            # :729-737: only images whose quota is above 0 run the NMS
            cand = torch.where(sample.counts[:, 2] > 0, sample.fg_counts, torch.zeros_like(sample.fg_counts))
            sel_index = torch.empty((B, K), dtype=torch.int64, device=dev)
            sel_counts = torch.empty((B,), dtype=torch.int32, device=dev)
            sel_scores = torch.empty((B, K), **f32)
            check(lib.gnms_select_topk(ptr(scores), B, R, ptr(sample.fg_index), R, ptr(cand), K, None, ptr(sel_index), ptr(sel_counts),
                                       ptr(sel_scores), None, st), "gnms_select_topk")
            boxes = torch.empty((B, K, 4), **f32)
            cuboids = torch.empty((B, K, 7), **f32)
            gt_params = torch.empty((B, M, 7), **f32)
            gt_boxes = torch.empty((B, M, 4), **f32)
            check(lib.gnms_after_nms_decode(ptr(sel_index), ptr(sel_counts), B, K, R, ptr(x2), ptr(x3), D3, ptr(raw_gt), ld_gt, ptr(rois), ld_rois,
                                            ptr(rois_3d), ld_r3, ptr(cen), ptr(p2), int(p2.shape[1]), ptr(scale), ctypes.addressof(c_means),
                                            ctypes.addressof(c_stds), ptr(gv), ptr(g3), ld_g3, M, ptr(vc), ptr(boxes), ptr(cuboids),
                                            ptr(gt_params), ptr(gt_boxes), st), "gnms_after_nms_decode")
            nms_boxes = boxes
            if diff_nms_boxes_2d == "projected":          # :746-768, :774
                P = torch.zeros((B, 4, 4), **f32)
                P[:, 3, 3] = 1.0
                P[:, :p2.shape[1]] = p2.to(torch.float32)
                nms_boxes = torch.empty((B, K, 4), **f32)
                check(lib.gnms_project_boxes3d(ptr(cuboids), ptr(P), ptr(scale.to(torch.float32)), B, K, ptr(nms_boxes), st),
                      "gnms_project_boxes3d")
            # :772-793: the layer on the 2D overlaps of the selected boxes; the overlap matrix takes no gradient
            with torch.enable_grad():
                s_in = sel_scores.requires_grad_(True)
                out = G.differentiable_nms_with_iou2d_batched(s_in, nms_boxes, counts=sel_counts, nms_threshold=nms_threshold,
                                                              pruning_method=pruning_method, temperature=temperature,
                                                              valid_box_prob_threshold=valid_box_prob_threshold, return_sorted_prob=False,
                                                              group_boxes=group_boxes, mask_group_boxes=mask_group_boxes,
                                                              group_size=int(min(int(group_size), 2 ** 31 - 2)), index_lists=False)
                prob_nms = out[0]
            pn = prob_nms.detach().contiguous()
            # :801-825
            # (the index per ground truth only: the targets are filled by the finish kernel with plain stores)
            tg = torch.empty((B, K), **f32)
            best = torch.empty((B, M), dtype=torch.int64, device=dev)
            check(lib.gnms_best_targets(ptr(cuboids), ptr(boxes), ptr(gt_params), ptr(gt_boxes), B, K, M, ptr(sel_counts), ptr(vc),
                                        float(best_target_box_beta), ptr(best), None, None, st), "gnms_best_targets")
            # :1091-1148
            tail = torch.empty((B + 1,), dtype=torch.int32, device=dev)
            tg_pad = torch.empty((B, K), **f32)
            ap_loss = torch.empty((B,), **f32)
            ap_grad = torch.empty((B, K), **f32)
            out_loss = torch.empty((2 + B,), **f32)
            img_cnt = torch.empty((1,), dtype=torch.int32, device=dev)
            dpn = torch.empty((B, K), **f32)
            lam = float(after_nms_lambda)
            check(lib.gnms_after_nms_finish(0, mode, B, K, ptr(sample.fg_counts), ptr(sel_counts), ptr(pn), ptr(tg), None, None, lam, ptr(tail),
                                            ptr(tg_pad), None, None, None, ptr(best), M, st), "gnms_after_nms_finish")
            if mode == 0:
                check(lib.gnms_aploss_tail(ptr(pn), ptr(tg), B, K, ptr(sel_counts), ptr(tail), 1.0, 0.0, ptr(ap_loss), ptr(ap_grad), st),
                      "gnms_aploss_tail")
            elif mode == 1:
                check(lib.gnms_aploss_tail(ptr(pn), ptr(tg_pad), 1, B * K, None, ptr(tail[B:]), 1.0, 0.0, ptr(ap_loss), ptr(ap_grad), st),
                      "gnms_aploss_tail")
            check(lib.gnms_after_nms_finish(1, mode, B, K, ptr(sample.fg_counts), ptr(sel_counts), ptr(pn), ptr(tg), ptr(ap_loss), ptr(ap_grad),
                                            lam, None, None, ptr(out_loss), ptr(img_cnt), ptr(dpn), None, 0, st), "gnms_after_nms_finish")
            # the layer's backward, then the scatter into the heads' dense gradients
            (dscore,) = torch.autograd.grad(prob_nms, s_in, dpn)
            dscore = dscore.to(torch.float32).contiguous()
            dacc = torch.empty((B, R), **f32) if xa is not None else None
            dprob = torch.empty((B, R, C), **f32) if use_prob else None
            check(lib.gnms_after_nms_scatter(ptr(sel_index), ptr(sel_counts), ptr(dscore), B, K, R, max(C, 2), ptr(xa), ptr(xp), ptr(cls_pred),
                                             ptr(dacc), ptr(dprob), st), "gnms_after_nms_scatter")
        info[STAT_NAME[after_nms_loss_mode]] = out_loss[1]
        info["sel_index"], info["sel_counts"] = sel_index, sel_counts
        info["scores_after_nms"], info["targets_after_nms"] = pn, tg
        info["losses"] = out_loss[2:]
        info["img_cnt"] = img_cnt.reshape(())
        return out_loss[0], dacc, dprob

    return run, info, use_prob


def after_nms_loss(prob, acceptance, bbox_2d, bbox_3d, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, gts_val, gts_3d,
                   val_counts, *, means, stds, after_nms_lambda=0.05, after_nms_loss_mode="rank", rank_boxes_of_all_images_at_once=False,
                   rank_with_class_confidence=False, best_target_box_beta=0.3, nms_threshold=0.4, pruning_method="linear", temperature=0.1,
                   valid_box_prob_threshold=0.3, group_boxes=True, mask_group_boxes=True, group_size=100, diff_nms_boxes_2d="normal",
                   overlap_in_nms="2d", max_nms_boxes=500, decomp_alpha=True):
    """prob [B, R, C] (column 0 = background), acceptance [B, R] or None, bbox_2d [B, R, 4], bbox_3d [B, R, >= 10]: the heads.  targets:
    Targets of compute_targets_batched or a (transforms, raw_gt) pair (raw_gt [B, R, >= 21] is read where it lies, with a row stride);
    sample: Sample of sample_anchors; rois [B, R, >= 4], rois_3d [B, R, >= 11], rois_3d_cen [B, R, 2]; p2 [B, 3 or 4, 4] and
    scale_factor [B] (float64 on the device); gts_val [B, M, 4], gts_3d [B, M, >= 11], val_counts [B] as compute_targets_batched takes
    them (the cuboid of a ground truth is columns 7, 8, 9, 3, 4, 5, 10).  means / stds: 13 host values each.
    The score of an anchor is acceptance (times max(prob[1:]) with rank_with_class_confidence, one fp32 product), or max(prob[1:])
    without an acceptance head.  Images with sample.counts[b, 2] > 0 (the quota) send the min(max_nms_boxes, fg_counts[b]) best of
    sample.fg_index[b, :fg_counts[b]] through the NMS.
    -> (loss, info): loss a scalar tensor, differentiable w.r.t. acceptance (and prob where the scores read it); info a dict of device
    tensors: the statistic under the reference's name (bbox_after_nms_rank / bbox_after_nms_class), sel_index [B, K] int64 (-1 behind
    sel_counts [B]), scores_after_nms / targets_after_nms [B, K] in selection order, losses [B] (the per-image AP losses; 0 in the other
    modes) and img_cnt (int32 scalar).  Without sampled foreground in the batch: loss 0, gradients 0."""
    run, info, use_prob = _after_nms_term(prob, acceptance, bbox_2d, bbox_3d, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, gts_val,
                                          gts_3d, val_counts, means=means, stds=stds, after_nms_lambda=after_nms_lambda,
                                          after_nms_loss_mode=after_nms_loss_mode,
                                          rank_boxes_of_all_images_at_once=rank_boxes_of_all_images_at_once,
                                          rank_with_class_confidence=rank_with_class_confidence, best_target_box_beta=best_target_box_beta,
                                          nms_threshold=nms_threshold, pruning_method=pruning_method, temperature=temperature,
                                          valid_box_prob_threshold=valid_box_prob_threshold, group_boxes=group_boxes,
                                          mask_group_boxes=mask_group_boxes, group_size=group_size, diff_nms_boxes_2d=diff_nms_boxes_2d,
                                          overlap_in_nms=overlap_in_nms, max_nms_boxes=max_nms_boxes, decomp_alpha=decomp_alpha)
    loss = _AfterNMSLoss.apply(run, acceptance, prob if use_prob else None)
    return loss, info
