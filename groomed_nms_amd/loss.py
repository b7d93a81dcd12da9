"""The reference's detection loss as one device-resident module (csrc/loss.hip): lib/loss/rpn_3d.py's RPN_3D_loss with its
call signature, from the ground-truth objects to the total, the `stats` list and the gradients of the five heads.

  pack_ground_truths   the only host work of a step: the batch's ground truths as one pinned record array (GroundTruths), in the order
                       the reference iterates them; GroundTruths.to uploads it with one copy
  RPN_3D_loss          forward(cls, prob, bbox_2d, bbox_3d, imobjs, feat_size, rois, rois_3d, rois_3d_cen, bbox_acceptance_prob) as
                       scripts/train_rpn_3d.py:140 calls it = pack_ground_truths + GroundTruths.to + forward_packed
  forward_packed       device tensors in, device tensors out: gnms_gt_filter (:399-419) -> targets.compute_targets_batched ->
                       sampling.sample_anchors -> the classification, after-NMS and regression terms (the launches of
                       classification_loss, after_nms_loss and regression_loss, shared with them) -> gnms_loss_combine.  One
                       autograd.Function wraps all of it; its backward is one launch, gnms_loss_grad_combine.  Stream-ordered, nothing
                       is read back: capturable in a graph together with loss.backward().

`stats` is the reference's list of {'name', 'val', 'format', 'group'} in the reference's order; every `val` is a zero-dimensional view
into one float64 vector, `module.last_stats` (STATS_LAYOUT names its entries).  lib/core.py:compute_stats works on the list unchanged
(one device-to-host read per entry); one read of `last_stats` serves them all.

Deliberate differences from the reference:
  * nothing is read back to decide what to append: the entries of a configured term are always in the list, where the reference omits
    `fg` / `bg` without such a label, `cls` without an active anchor, everything from `bbox_2d` to `total` without sampled foreground
    (the regression statistics are then NaN, `total` is the sum of the other terms), `un` and `conf` while the running uncertainty
    weight is 0, and `iou_2d_los` when every IoU is 0 (it is 0 then).
  * inherited from the five calls: ties among equal scores at a sampling quota or at the cut to 500 boxes go to the lower anchor index;
    an element that an isfinite filter drops gets gradient 0 where the reference's backward yields NaN; bbox_2d is read as the network
    gave it (the reference's bbox_transform_inv has scaled it in place before the 2D term reads it; equal for 2D means 0 and stds 1);
    the AP loss adds in selection order.
  * max_gt_h is not applied, as in the reference (its call of determine_ignores leaves the default 10e10).
There is no CPU implementation here.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from . import after_nms, heads, regression, sampling, targets

__all__ = ["RPN_3D_loss", "pack_ground_truths", "GroundTruths", "RECORD_COLS", "STATS_LAYOUT"]

RECORD_COLS = 24           # GNMS_LOSS_RECORD_COLS: bbox_full [0..3], bbox_3d [4..19], class id [20], ign [21], visibility [22], trunc [23]
MAX_GTS = 256              # GNMS_LOSS_MAX_GTS
MAX_GT_H = 10e10           # rpn_util.py:937: the loss calls determine_ignores without max_gt_h
# GNMS_LOSS_STATS: the entries of last_stats; all but the last in the order of the reference's stats.append calls (:903 to :1407)
STATS_LAYOUT = ("fg", "bg", "cls", "after_nms", "bbox_2d", "cen", "cen_dist_lt_0.2", "axis", "head", "conf", "bbox_3d", "un", "z", "rot", "iou_2d",
                "iou_2d_los", "total", "bbox_un_lambda")
_FORMATS = {"fg": ("{:0.2f}", "acc"), "bg": ("{:0.2f}", "acc"), "cls": ("{:0.4f}", "loss"), "after_nms": ("{:0.4f}", "loss"),
            "bbox_2d": ("{:0.4f}", "loss"), "cen": ("{:0.2f}", "misc"), "cen_dist_lt_0.2": ("{:0.3f}", "misc"), "axis": ("{:0.2f}", "acc"),
            "head": ("{:0.2f}", "acc"), "conf": ("{:0.2f}", "misc"), "bbox_3d": ("{:0.4f}", "loss"), "un": ("{:0.4f}", "loss"),
            "z": ("{:0.2f}", "misc"), "rot": ("{:0.2f}", "misc"), "iou_2d": ("{:0.2f}", "acc"), "iou_2d_los": ("{:0.4f}", "loss"),
            "total": ("{:0.4f}", "loss")}


def _field(obj, name, default=None):
    """a field of an easydict-like object, by attribute or by key"""
    if isinstance(obj, dict):
        return obj.get(name, default)
    return getattr(obj, name, default)


class GroundTruths:
    """The ground truths of a batch in ONE float64 buffer: records [B, capacity, RECORD_COLS], p2 [B, 4, 4], scale_factor [B] and, in the
    buffer's last ceil(B / 2) elements, counts [B] as int32 -- views of `buffer`, so one copy moves them all."""

    def __init__(self, buffer, batch, capacity):
        B, cap = int(batch), int(capacity)
        n_rec, n_cnt = B * cap * RECORD_COLS, (B + 1) // 2
        if buffer.dtype != torch.float64 or buffer.dim() != 1 or buffer.numel() != self.elements(B, cap) or not buffer.is_contiguous():
            raise ValueError("buffer must be a contiguous float64 vector of %d elements" % self.elements(B, cap))
        self.buffer, self.batch, self.capacity = buffer, B, cap
        self.records = buffer[:n_rec].view(B, cap, RECORD_COLS)
        self.p2 = buffer[n_rec:n_rec + 16 * B].view(B, 4, 4)
        self.scale_factor = buffer[n_rec + 16 * B:n_rec + 17 * B]
        self.counts = buffer[n_rec + 17 * B:n_rec + 17 * B + n_cnt].view(torch.int32)[:B]

    @staticmethod
    def elements(batch, capacity):
        return batch * capacity * RECORD_COLS + 17 * batch + (batch + 1) // 2

    @classmethod
    def empty(cls, batch, capacity, device=None, pin_memory=False):
        return cls(torch.empty(cls.elements(batch, capacity), dtype=torch.float64, device=device, pin_memory=pin_memory), batch, capacity)

    def to(self, device, non_blocking=True, out=None):
        """one copy of the buffer -> the GroundTruths on `device`.  out: a GroundTruths there (GroundTruths.empty(B, capacity, device)) to copy
        into, so that the device addresses stay the same from step to step (a captured graph reads them); None: a new one"""
        if out is None:
            out = GroundTruths.empty(self.batch, self.capacity, device=device)
        if (out.batch, out.capacity) != (self.batch, self.capacity) or out.buffer.device != torch.device(device):
            raise ValueError("out holds [%d, %d] on %s, not [%d, %d] on %s" % (out.batch, out.capacity, out.buffer.device, self.batch, self.capacity,
                                                                            torch.device(device)))
        out.buffer.copy_(self.buffer, non_blocking=non_blocking)
        return out


def pack_ground_truths(imobjs, lbls, ilbls, key="gts", capacity=64):
    """imobjs: per image an object with [key] (the ground truths: cls, ign, visibility, trunc, bbox_full [4], bbox_3d [16]), p2 (3 or 4 rows)
    and scale_factor.  -> GroundTruths on the host (pinned where a GPU is present): one row per ground truth in the reference's order,
    the class id 1 + index in lbls, 0 for a class of ilbls (which the reference ignores whatever lbls says), -1 for neither (removed).
    Rows behind counts[b] are zero.  More than `capacity` ground truths in an image: ValueError."""
    B, cap = len(imobjs), int(capacity)
    if not 1 <= cap <= MAX_GTS:
        raise ValueError("capacity must be 1..%d, got %d" % (MAX_GTS, cap))
    gt = GroundTruths.empty(B, cap, pin_memory=torch.cuda.is_available())
    buf = gt.buffer.numpy()
    buf[:] = 0.0
    rec = buf[:B * cap * RECORD_COLS].reshape(B, cap, RECORD_COLS)
    p2 = buf[B * cap * RECORD_COLS:][:16 * B].reshape(B, 4, 4)
    scale = buf[B * cap * RECORD_COLS + 16 * B:][:B]
    counts = gt.counts.numpy()
    ids = {name: 1.0 + i for i, name in enumerate(lbls)}
    ids.update({name: 0.0 for name in ilbls})
    for b, imobj in enumerate(imobjs):
        gts = _field(imobj, key)
        if len(gts) > cap:
            raise ValueError("image %d has %d ground truths, capacity is %d" % (b, len(gts), cap))
        for j, g in enumerate(gts):
            row = rec[b, j]
            row[0:4] = np.asarray(_field(g, "bbox_full"), np.float64)[:4]
            b3 = np.asarray(_field(g, "bbox_3d"), np.float64).reshape(-1)[:16]
            row[4:4 + len(b3)] = b3
            row[20] = ids.get(_field(g, "cls"), -1.0)
            row[21] = 1.0 if _field(g, "ign", False) else 0.0
            row[22] = _field(g, "visibility", 1.0)
            row[23] = _field(g, "trunc", 0.0)
        counts[b] = len(gts)
        m = np.asarray(_field(imobj, "p2"), np.float64)
        if m.shape not in ((3, 4), (4, 4)):
            raise ValueError("image %d: p2 must be [3 or 4, 4], got %s" % (b, m.shape))
        p2[b, 3] = (0.0, 0.0, 0.0, 1.0)
        p2[b, :m.shape[0]] = m
        scale[b] = float(_field(imobj, "scale_factor", 1.0))
    return gt


class _Loss(torch.autograd.Function):
    """total = gnms_loss_combine's scalar; the terms wrote their dense gradients in the forward, and the backward scales them into the
    five heads' gradients in one launch"""

    @staticmethod
    def forward(ctx, run, cls, prob, bbox_2d, bbox_3d, acceptance):
        total, g = run()
        ctx.names = [k for k in ("dcls", "dprob", "d2", "d3", "da", "dacc") if g.get(k) is not None]
        ctx.save_for_backward(*[g[k] for k in ctx.names])
        ctx.like = [(t.dtype, tuple(t.shape)) if t is not None else None for t in (cls, prob, bbox_2d, bbox_3d, acceptance)]
        ctx.dev = total.device
        return total

    @staticmethod
    def backward(ctx, grad_output):
        g = dict(zip(ctx.names, ctx.saved_tensors))
        dev = ctx.dev
        need = ctx.needs_input_grad[1:]
        out = [torch.empty(like[1], dtype=torch.float32, device=dev) if like is not None and n else None for like, n in zip(ctx.like, need)]
        B, R, C = ctx.like[0][1]
        D3 = ctx.like[3][1][2]
        up = grad_output.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        lib = _lib.load()
        with _lib.on_device(dev):
            rc = lib.gnms_loss_grad_combine(ptr(up), B * R, C, D3, ptr(g.get("dcls")), ptr(g.get("dprob")), ptr(g.get("d2")), ptr(g.get("d3")),
                                            ptr(g.get("da")), ptr(g.get("dacc")), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]),
                                            stream_ptr(dev))
        check(rc, "gnms_loss_grad_combine")
        return (None,) + tuple(o.to(like[0]) if o is not None else None for o, like in zip(out, ctx.like))


def _as_batch(t, B, dev):
    """a table of the reference's call site ([R, .], [B, R, .] or more images than the batch has) as [B, R, .] on the device"""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    t = t.detach().to(dev)
    if t.dim() == 2:
        return t.unsqueeze(0).expand(B, -1, -1).contiguous()
    return t[:B]


class RPN_3D_loss(torch.nn.Module):
    """lib/loss/rpn_3d.py:17, on the GPU.  `conf` is read with the reference's defaults (:19-160); a branch the kernels do not implement
    raises NotImplementedError here, naming its key.  capacity: the most ground truths an image may carry (<= 256)."""

    def __init__(self, conf, verbose=True, *, capacity=64):
        super().__init__()

        def get(key, default):
            return conf[key] if key in conf else default
        self.lbls, self.ilbls = list(conf["lbls"]), list(conf["ilbls"])
        self.anchors = np.asarray(conf["anchors"], np.float64)
        self.bbox_means, self.bbox_stds = np.asarray(conf["bbox_means"], np.float64), np.asarray(conf["bbox_stds"], np.float64)
        for k in ("feat_stride", "fg_fraction", "box_samples", "ign_thresh", "nms_thres", "fg_thresh", "bg_thresh_lo", "bg_thresh_hi", "best_thresh",
                  "hard_negatives", "focal_loss", "cls_2d_lambda", "iou_2d_lambda", "bbox_2d_lambda", "bbox_3d_lambda", "min_gt_vis", "min_gt_h",
                  "max_gt_h"):
            setattr(self, k, conf[k])
        for k, d in (("bbox_axis_head_lambda", 0), ("has_un", 0), ("bbox_un_lambda", 0), ("decomp_alpha", False), ("bbox_un_dynamic", False),
                     ("infer_2d_from_3d", False), ("orientation_bins", False), ("use_nms_in_loss", False), ("diff_nms_pruning_method", "linear"),
                     ("diff_nms_temperature", 1), ("diff_nms_valid_box_prob_threshold", 0.3), ("diff_nms_boxes_2d", "normal"),
                     ("diff_nms_group_boxes", True), ("diff_nms_mask_group_boxes", True), ("diff_nms_group_size", 100), ("after_nms_lambda", 1),
                     ("after_nms_loss_mode", "rank"), ("overlap_in_nms", "2d"), ("predict_acceptance_prob", False), ("acceptance_prob_lambda", 0),
                     ("acceptance_prob_mode", "regress"), ("boxes_for_acceptance_prob", "all"), ("use_acceptance_prob_in_regression_loss", False),
                     ("rank_with_class_confidence", False), ("rank_boxes_of_all_images_at_once", False),
                     ("weigh_3D_regression_loss_by_gt_iou3d", False), ("best_target_box_beta", 0.3)):
            setattr(self, k, get(k, d))
        self.verbose = verbose
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= MAX_GTS:
            raise ValueError("capacity must be 1..%d, got %d" % (MAX_GTS, self.capacity))
        self.after_nms_on = bool(self.use_nms_in_loss and self.after_nms_lambda)
        for key, bad in (("has_un", bool(self.has_un)), ("orientation_bins", self.orientation_bins > 0), ("decomp_alpha", not self.decomp_alpha),
                         ("infer_2d_from_3d", bool(self.infer_2d_from_3d)), ("hard_negatives", not self.hard_negatives),
                         ("acceptance_prob_lambda", bool(self.predict_acceptance_prob and self.acceptance_prob_lambda)),
                         ("acceptance_prob_mode", self.acceptance_prob_mode == "classify"),
                         ("overlap_in_nms", self.overlap_in_nms != "2d"),
                         ("after_nms_loss_mode", self.after_nms_on and self.after_nms_loss_mode not in ("rank", "classify")),
                         ("weigh_3D_regression_loss_by_gt_iou3d", bool(self.weigh_3D_regression_loss_by_gt_iou3d)),
                         # :1003-1016: classify and rank-all read accept_prob_active; the after-NMS kernels take it as the sampled foreground
                         ("boxes_for_acceptance_prob", self.after_nms_on and self.boxes_for_acceptance_prob in ("all", "overlaps")
                          and (self.after_nms_loss_mode == "classify" or bool(self.rank_boxes_of_all_images_at_once)))):
            if bad:
                raise NotImplementedError("RPN_3D_loss: %s=%r is not implemented on the GPU (the supported branches: INTEGRATION.md 3c*)"
                                          % (key, get(key, None)))
        self.un_state = None                         # the reference's self.n_frames / self.bbox_un_lambda, on the device
        self.last_stats = None
        self._gt = {}                                # the device GroundTruths of forward(), per (device, B)

    # ------------------------------------------------------------------------------------------ the stats list
    def stat_entries(self):
        """[(name in the list, entry of last_stats)] in the reference's order, as `verbose` and the configuration gate them"""
        v = self.verbose
        acc_in_3d = bool(self.predict_acceptance_prob or self.use_acceptance_prob_in_regression_loss or self.bbox_un_dynamic)
        un = bool(self.bbox_un_dynamic or self.bbox_un_lambda > 0)
        gates = (("fg", bool(self.cls_2d_lambda)), ("bg", bool(self.cls_2d_lambda) and v), ("cls", bool(self.cls_2d_lambda)),
                 ("after_nms", self.after_nms_on), ("bbox_2d", bool(self.bbox_2d_lambda) and v), ("cen", v), ("cen_dist_lt_0.2", True),
                 ("axis", bool(self.bbox_3d_lambda) and v), ("head", bool(self.bbox_3d_lambda) and v), ("conf", bool(self.bbox_3d_lambda) and acc_in_3d),
                 ("bbox_3d", bool(self.bbox_3d_lambda)), ("un", un), ("z", True), ("rot", True), ("iou_2d", True),
                 ("iou_2d_los", bool(self.iou_2d_lambda) and v), ("total", True))
        names = dict(after_nms=after_nms.STAT_NAME.get(self.after_nms_loss_mode, "bbox_after_nms"))
        return [(names.get(k, k), k) for k, on in gates if on]

    def _stats_list(self, vec):
        return [{"name": name, "val": vec[STATS_LAYOUT.index(k)], "format": _FORMATS[k][0], "group": _FORMATS[k][1]} for name, k in self.stat_entries()]

    # ------------------------------------------------------------------------------------------ the calls
    def forward(self, cls, prob, bbox_2d, bbox_3d, imobjs, feat_size, rois=None, rois_3d=None, rois_3d_cen=None, bbox_acceptance_prob=None,
                bbox_acceptance_prob_cls=None, key="gts"):
        """the reference's signature (:162).  -> (loss, stats)"""
        if bbox_acceptance_prob_cls is not None:
            raise NotImplementedError("RPN_3D_loss: bbox_acceptance_prob_cls (acceptance_prob_mode='classify') is not implemented on the GPU")
        dev = cls.device
        B = int(cls.shape[0])
        host = pack_ground_truths(imobjs[:B], self.lbls, self.ilbls, key=key, capacity=self.capacity)
        slot = self._gt.get((dev, B))
        if slot is None:
            slot = self._gt[(dev, B)] = GroundTruths.empty(B, self.capacity, device=dev)
        gt = host.to(dev, non_blocking=True, out=slot)
        if rois is None or rois_3d is None or rois_3d_cen is None:
            grid = heads.anchor_grid(self.anchors, feat_size, self.feat_stride, batch=B, device=dev)
            rois = grid[0] if rois is None else rois
            rois_3d = grid[1] if rois_3d is None else rois_3d
            rois_3d_cen = grid[2] if rois_3d_cen is None else rois_3d_cen
        return self.forward_packed(cls, prob, bbox_2d, bbox_3d, gt, rois, rois_3d, rois_3d_cen, bbox_acceptance_prob)

    def forward_packed(self, cls, prob, bbox_2d, bbox_3d, gt, rois, rois_3d, rois_3d_cen, bbox_acceptance_prob=None):
        """cls, prob [B, R, C], bbox_2d [B, R, 4], bbox_3d [B, R, >= 10], bbox_acceptance_prob [B, R, 1] or None: the heads; gt: GroundTruths
        on their device; rois [B, R, >= 5] (or [R, .], as for the two others), rois_3d [B, R, >= 11], rois_3d_cen [B, R, 2].
        -> (loss, stats): loss a scalar tensor, differentiable w.r.t. the five heads; stats the reference's list (views of last_stats)."""
        dev = cls.device
        if dev.type != "cuda":
            raise ValueError("the heads must lie on a GPU (got %s); there is no CPU fallback" % dev)
        if cls.dim() != 3 or tuple(prob.shape) != tuple(cls.shape):
            raise ValueError("cls and prob must be [B, R, C], got %s and %s" % (tuple(cls.shape), tuple(prob.shape)))
        B, R, C = (int(v) for v in cls.shape)
        if gt.batch != B or gt.buffer.device != dev:
            raise ValueError("gt holds %d images on %s, the heads %d on %s" % (gt.batch, gt.buffer.device, B, dev))
        acc = bbox_acceptance_prob
        if acc is not None and tuple(acc.shape) != (B, R, 1):
            raise ValueError("bbox_acceptance_prob must be [B, R, 1] = [%d, %d, 1], got %s" % (B, R, tuple(acc.shape)))
        acc2 = acc[:, :, 0] if acc is not None else None
        rois, rois_3d, rois_3d_cen = (_as_batch(t, B, dev) for t in (rois, rois_3d, rois_3d_cen))
        if self.bbox_un_dynamic and (self.un_state is None or self.un_state.device != dev):
            self.un_state = regression.new_un_state(dev, 0, float(self.bbox_un_lambda))
        lib = _lib.load()
        cap = gt.capacity
        means, stds = self.bbox_means.reshape(-1), self.bbox_stds.reshape(-1)
        stats = torch.empty((len(STATS_LAYOUT),), dtype=torch.float64, device=dev)

        def run():
            st = stream_ptr(dev)
            f64 = dict(dtype=torch.float64, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            gts_val, gts_ign = torch.empty((B, cap, 4), **f64), torch.empty((B, cap, 4), **f64)
            gts_3d, box_lbls = torch.empty((B, cap, 16), **f64), torch.empty((B, cap), **i32)
            val_counts, ign_counts = torch.empty((B,), **i32), torch.empty((B,), **i32)
            with _lib.on_device(dev):                  # :399-419
                check(lib.gnms_gt_filter(ptr(gt.records), ptr(gt.counts), B, cap, float(self.min_gt_vis), float(self.min_gt_h), MAX_GT_H, 0, ptr(gts_val),
                                         ptr(box_lbls), ptr(gts_3d), ptr(gts_ign), ptr(val_counts), ptr(ign_counts), st), "gnms_gt_filter")
            t = targets.compute_targets_batched(rois, gts_val, box_lbls, self.fg_thresh, self.ign_thresh, self.bg_thresh_lo, self.bg_thresh_hi,
                                                self.best_thresh, gts_ign=gts_ign, val_counts=val_counts, ign_counts=ign_counts, gts_3d=gts_3d,
                                                rois_3d=rois_3d, rois_3d_cen=rois_3d_cen, anchor_cols=self.anchors.shape[1], means=means, stds=stds,
                                                want=("transforms", "raw_gt"))          # :435-453
            s = sampling.sample_anchors(t.transforms[..., 4], prob, val_counts, box_samples=self.box_samples, fg_fraction=self.fg_fraction,
                                        hard_negatives=self.hard_negatives)
            g = {}
            cls_loss = cls_acc = after = None
            if self.cls_2d_lambda:                     # :893-907, :913-1001
                run_cls, cls_acc = sampling._cls_term(cls, s, fg_fraction=self.fg_fraction, focal_loss=self.focal_loss, cls_2d_lambda=self.cls_2d_lambda)
                cls_loss, g["dcls"] = run_cls(cls.detach())
            if self.after_nms_on:                      # :721-825, :1091-1148
                run_nms, _, _ = after_nms._after_nms_term(
                    prob, acc2, bbox_2d, bbox_3d, t, s, rois, rois_3d, rois_3d_cen, gt.p2, gt.scale_factor, gts_val, gts_3d, val_counts, means=means,
                    stds=stds, after_nms_lambda=self.after_nms_lambda, after_nms_loss_mode=self.after_nms_loss_mode,
                    rank_boxes_of_all_images_at_once=self.rank_boxes_of_all_images_at_once, rank_with_class_confidence=self.rank_with_class_confidence,
                    best_target_box_beta=self.best_target_box_beta, nms_threshold=self.nms_thres, pruning_method=self.diff_nms_pruning_method,
                    temperature=self.diff_nms_temperature, valid_box_prob_threshold=self.diff_nms_valid_box_prob_threshold,
                    group_boxes=self.diff_nms_group_boxes, mask_group_boxes=self.diff_nms_mask_group_boxes, group_size=self.diff_nms_group_size,
                    diff_nms_boxes_2d=self.diff_nms_boxes_2d, overlap_in_nms=self.overlap_in_nms, decomp_alpha=self.decomp_alpha)
                after, g["dacc"], g["dprob"] = run_nms()
            run_reg, reg_stats, reg_counts = regression._reg_term(                      # :1154-1407
                bbox_2d, bbox_3d, acc2, t, s, rois, rois_3d, rois_3d_cen, gt.p2, gt.scale_factor, means=means, stds=stds,
                bbox_2d_lambda=self.bbox_2d_lambda, bbox_3d_lambda=self.bbox_3d_lambda, bbox_axis_head_lambda=self.bbox_axis_head_lambda,
                iou_2d_lambda=self.iou_2d_lambda, use_acceptance_prob_in_regression_loss=self.use_acceptance_prob_in_regression_loss,
                bbox_un_lambda=self.bbox_un_lambda, bbox_un_dynamic=self.bbox_un_dynamic, un_state=self.un_state)
            _, g["d2"], g["d3"], g["da"] = run_reg()
            total = torch.empty((1,), dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                check(lib.gnms_loss_combine(ptr(cls_loss), ptr(cls_acc), ptr(after), ptr(reg_stats), ptr(reg_counts), ptr(total), ptr(stats), st),
                      "gnms_loss_combine")
            self.last_sample = s
            self.last_ground_truths = dict(gts_val=gts_val, gts_ign=gts_ign, gts_3d=gts_3d, box_lbls=box_lbls, val_counts=val_counts, ign_counts=ign_counts)
            return total.reshape(()), g

        loss = _Loss.apply(run, cls, prob, bbox_2d, bbox_3d, acc)
        self.last_stats = stats
        return loss, self._stats_list(stats)
