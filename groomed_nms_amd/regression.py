"""Box regression, 2D IoU and uncertainty terms of the RPN loss on the GPU (csrc/regression.hip): what
lib/loss/rpn_3d.py does with the sampled foreground, on top of targets.compute_targets_batched and sampling.sample_anchors.

  regression_loss   :1163-1191 (2D smooth-L1), :1211-1373 (3D smooth-L1 with the sin / cos choice, axis and head cross entropies, the
                    running uncertainty weight, the acceptance weighting), :1375-1382 (uncertainty term), :1390-1405 (-log IoU), and
                    the cen / z / rot / iou_2d / axis / head / conf statistics (:318-357, :532-577, :1194-1209, :1384-1392)
Device tensors in, device tensors out; nothing is read back and both launches are stream-ordered, so the call can be captured in a graph
together with sample_anchors and classification_loss.  There is no CPU implementation here.

Two deliberate differences from the reference:
  * its bbox_transform_inv has overwritten bbox_2d with the denormalised deltas (rpn_util.py:902-912) before the 2D term reads it, so that
    term compares a denormalised prediction with a normalised target; here the prediction is used as the network gave it.  The two
    agree when the 2D means are 0 and the 2D stds are 1.
  * an element that an isfinite filter drops (:1358-1364, :1400) gets gradient 0; the reference's backward yields 0 * inf = NaN there,
    for example on a sampled box that misses its target.
The reference decodes every image's 2D prediction with rois[0] (:316); here image b uses rois[b].  The loss's call sites pass one anchor
grid for all images, so nothing differs.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

__all__ = ["regression_loss", "STAT_NAMES", "new_un_state"]

STAT_NAMES = ("bbox_2d", "bbox_3d", "un", "iou_2d_los", "cen", "cen_dist_lt_0.2", "z", "rot", "iou_2d", "axis", "head", "conf", "total",
              "bbox_un_lambda")
N_STATS, N_STAT_COUNTS = 14, 24            # GNMS_REG_STATS, GNMS_REG_STAT_COUNTS


def new_un_state(device, n_frames=0, weight=0.0):
    """the caller-owned state of bbox_un_dynamic: [n_frames, weight] float64 on `device` (the reference's self.n_frames, self.bbox_un_lambda)"""
    return torch.tensor([float(n_frames), float(weight)], dtype=torch.float64, device=device)


class _RegLoss(torch.autograd.Function):
    """loss = the kernel's scalar; its gradients w.r.t. the heads were written by the same call and are only scaled here"""

    @staticmethod
    def forward(ctx, run, bbox_2d, bbox_3d, acceptance):
        loss, d2, d3, da = run()
        ctx.save_for_backward(d2, d3, da if da is not None else d2.new_empty(0))
        ctx.like = [(t.dtype, t.shape) if t is not None else None for t in (bbox_2d, bbox_3d, acceptance)]
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        grads = []
        for g, like in zip(ctx.saved_tensors, ctx.like):
            grads.append((g * grad_output).to(like[0]).reshape(like[1]) if like is not None else None)
        return (None,) + tuple(grads)


def _rows(t, dev, B, R, min_cols, what):
    """[B, R, >= min_cols] float32 rows read where they lie: -> (tensor, the stride between anchors)"""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != B or t.shape[1] != R or t.shape[2] < min_cols:
        raise ValueError("%s must be [B, R, >= %d] = [%d, %d, >= %d], got %s"
                         % (what, min_cols, B, R, min_cols, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    t = t.detach().to(device=dev, dtype=torch.float32)
    if not (t.stride(2) == 1 and t.stride(1) >= t.shape[2] and (B == 1 or t.stride(0) == R * t.stride(1))):
        t = t.contiguous()
    return t, t.stride(1)


def _reg_term(bbox_2d, bbox_3d, acceptance, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, *, means, stds,
              bbox_2d_lambda=0.0, bbox_3d_lambda=1.0, bbox_axis_head_lambda=0.35, iou_2d_lambda=1.0,
              use_acceptance_prob_in_regression_loss=False, bbox_un_lambda=0.0, bbox_un_dynamic=False, un_state=None,
              decomp_alpha=True, orientation_bins=0, infer_2d_from_3d=False, has_un=False,
              weigh_3D_regression_loss_by_gt_iou3d=False):
    """regression_loss up to the launch -> (run, stats, stat_counts): run() launches gnms_reg_loss on the detached heads and returns
    (loss [], d2 [B, R, 4], d3 [B, R, D3], da [B, R] or None); stats [14] float64 and stat_counts [24] int32 are filled by it.  (Shared with
    loss.RPN_3D_loss, which scales the gradients in its one backward launch.)"""
    if not decomp_alpha or orientation_bins or infer_2d_from_3d or has_un or weigh_3D_regression_loss_by_gt_iou3d:
        raise NotImplementedError("regression_loss implements decomp_alpha=True, orientation_bins=0, infer_2d_from_3d=False, has_un=False, "
                                  "weigh_3D_regression_loss_by_gt_iou3d=False")
    use_acc = bool(use_acceptance_prob_in_regression_loss)
    dynamic = bool(bbox_un_dynamic)
    bbox_un_lambda = float(bbox_un_lambda)
    if acceptance is None and (use_acc or dynamic or bbox_un_lambda > 0):
        raise ValueError("the acceptance weighting and the uncertainty term need `acceptance`")
    if dynamic and un_state is None:
        raise ValueError("bbox_un_dynamic needs un_state (new_un_state(device))")
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
    if tuple(sample.fg_index.shape) != (B, R) or sample.fg_counts.numel() != B or tuple(sample.counts.shape) != (B, 6):
        raise ValueError("sample does not belong to heads of [B, R] = [%d, %d]" % (B, R))
    if any(t.dtype != torch.int32 or not t.is_contiguous() for t in (sample.fg_index, sample.fg_counts, sample.counts)):
        raise ValueError("sample.fg_index, fg_counts and counts must be contiguous int32 tensors (sample_anchors' outputs)")
    transforms, raw_gt = (targets.transforms, targets.raw_gt) if hasattr(targets, "transforms") else targets
    dev = sample.fg_index.device
    transforms, ld_tr = _rows(transforms, dev, B, R, 14, "targets.transforms")
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
    if dynamic and (un_state.dtype != torch.float64 or un_state.numel() != 2 or un_state.device != dev or not un_state.is_contiguous()):
        raise ValueError("un_state must be a contiguous float64 [2] tensor on %s" % dev)
    if not dev.type == "cuda" or any(t.device != dev for t in (sample.fg_counts, sample.counts)):
        raise ValueError("sample must lie on one GPU (got %s); there is no CPU fallback" % dev)
    lib = _lib.load()
    D3 = int(bbox_3d.shape[2])
    stats = torch.empty((N_STATS,), dtype=torch.float64, device=dev)
    stat_counts = torch.empty((N_STAT_COUNTS,), dtype=torch.int32, device=dev)
    c_means = (ctypes.c_double * 13)(*means[:13])
    c_stds = (ctypes.c_double * 13)(*stds[:13])

    def run():
        x2 = bbox_2d.detach().to(device=dev, dtype=torch.float32).contiguous()
        x3 = bbox_3d.detach().to(device=dev, dtype=torch.float32).contiguous()
        xa = acceptance.detach().to(device=dev, dtype=torch.float32).contiguous() if acceptance is not None else None
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        d2 = torch.empty((B, R, 4), dtype=torch.float32, device=dev)
        d3 = torch.empty((B, R, D3), dtype=torch.float32, device=dev)
        da = torch.empty((B, R), dtype=torch.float32, device=dev) if xa is not None else None
        wsb = lib.gnms_reg_loss_workspace_bytes(B, R)
        ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.gnms_reg_loss(ptr(x2), ptr(x3), D3, ptr(xa), ptr(transforms), ld_tr, ptr(raw_gt), ld_gt, ptr(rois), ld_rois, ptr(rois_3d),
                                   ld_r3, ptr(cen), ptr(p2), int(p2.shape[1]), ptr(scale), ptr(sample.fg_index), ptr(sample.fg_counts),
                                   ptr(sample.counts), B, R, ctypes.addressof(c_means), ctypes.addressof(c_stds),
                                   float(bbox_2d_lambda), float(bbox_3d_lambda), float(bbox_axis_head_lambda), float(iou_2d_lambda),
                                   int(use_acc), 0.0 if math.isnan(bbox_un_lambda) else bbox_un_lambda, int(dynamic),
                                   ptr(un_state) if dynamic else None, ptr(loss), ptr(stats), ptr(stat_counts), ptr(d2), ptr(d3), ptr(da),
                                   ptr(ws), wsb, stream_ptr(dev))
        check(rc, "gnms_reg_loss")
        return loss.reshape(()), d2, d3, da

    return run, stats, stat_counts


def regression_loss(bbox_2d, bbox_3d, acceptance, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, *, means, stds,
                    bbox_2d_lambda=0.0, bbox_3d_lambda=1.0, bbox_axis_head_lambda=0.35, iou_2d_lambda=1.0,
                    use_acceptance_prob_in_regression_loss=False, bbox_un_lambda=0.0, bbox_un_dynamic=False, un_state=None,
                    decomp_alpha=True, orientation_bins=0, infer_2d_from_3d=False, has_un=False,
                    weigh_3D_regression_loss_by_gt_iou3d=False):
    """bbox_2d [B, R, 4], bbox_3d [B, R, >= 10] (x, y, z, w, h, l, rsin, rcos, axis, head; further columns get gradient 0), acceptance
    [B, R] or None: the heads, differentiable.  targets: Targets of compute_targets_batched (normalised transforms [B, R, >= 14], raw_gt
    [B, R, >= 21]; views with a row stride are read where they lie) or a (transforms, raw_gt) pair; sample: Sample of sample_anchors;
    rois [B, R, >= 4], rois_3d [B, R, >= 11], rois_3d_cen [B, R, 2]; p2 [B, 3 or 4, 4] and scale_factor [B] (float64 on the device).
    means / stds: 13 host values each (conf.bbox_means[0], conf.bbox_stds[0]).  With bbox_un_dynamic, un_state is the caller-owned
    device state of new_un_state(); it is advanced by the call, on the device.
    -> (loss, stats): loss a scalar tensor, differentiable w.r.t. the three heads; stats a dict of device scalars (float64) named as the
    reference's (STAT_NAMES), `total` being the sum of these terms and `bbox_un_lambda` the uncertainty weight in use, plus `counts`
    (int32 [24], GNMS_REG_STAT_COUNTS).  Without an active anchor in the batch: loss 0, gradients 0, statistics NaN, un_state untouched.
    See the module's docstring for the two deliberate differences from the reference and for rois[b]."""
    run, stats, stat_counts = _reg_term(bbox_2d, bbox_3d, acceptance, targets, sample, rois, rois_3d, rois_3d_cen, p2, scale_factor, means=means,
                                        stds=stds, bbox_2d_lambda=bbox_2d_lambda, bbox_3d_lambda=bbox_3d_lambda,
                                        bbox_axis_head_lambda=bbox_axis_head_lambda, iou_2d_lambda=iou_2d_lambda,
                                        use_acceptance_prob_in_regression_loss=use_acceptance_prob_in_regression_loss,
                                        bbox_un_lambda=bbox_un_lambda, bbox_un_dynamic=bbox_un_dynamic, un_state=un_state,
                                        decomp_alpha=decomp_alpha, orientation_bins=orientation_bins, infer_2d_from_3d=infer_2d_from_3d,
                                        has_un=has_un, weigh_3D_regression_loss_by_gt_iou3d=weigh_3D_regression_loss_by_gt_iou3d)
    loss = _RegLoss.apply(run, bbox_2d, bbox_3d, acceptance)
    out = {name: stats[i] for i, name in enumerate(STAT_NAMES)}
    out["counts"] = stat_counts
    return loss, out
