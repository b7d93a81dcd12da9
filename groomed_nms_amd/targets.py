"""Anchor training targets on the GPU (csrc/targets.hip).

  compute_targets           lib/rpn_util.py:411-524, same name, signature, shapes and dtypes: NumPy in, NumPy out.  It covers both
                            callers, the loss (lib/loss/rpn_3d.py:435, float32 rois, rois_3d + rois_3d_cen) and the statistics pass
                            (lib/rpn_util.py:620-699, float64 rois, anchors[tracker] as the 3D source).
  compute_targets_batched   B images of device tensors with ragged ground-truth counts and, optionally, the call site's normalisation
                            (rpn_3d.py:440-451) fused; device tensors out, no host round trip.
The arithmetic follows NumPy's type promotion bit for bit (roi-only terms in the rois' dtype, everything with a ground truth in
float64, one rounding into the float32 outputs).  There is no CPU implementation here.

One deliberate difference: the reference's 2D-only call (lib/rpn_util.py:626) leaves `anchors` at its default `[]`, and
`anchors.shape` then raises.  Here `anchors=None` or an empty sequence means "no decomp_alpha, no velocity".
"""
import collections

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, on_device

__all__ = ["compute_targets", "compute_targets_batched", "Targets", "MAX_GTS"]

MAX_GTS = 256         # GNMS_TARGETS_MAX_GTS: ground truths and ignore boxes per image

Targets = collections.namedtuple("Targets", ["transforms", "raw_gt", "ols_max", "ols", "ols_ign", "best_roi"])


def _device():
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _f64_host(v, n, what):
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1))
    if a.size < n:
        raise ValueError("%s: %d values, the normalisation needs %d" % (what, a.size, n))
    return a[:n].copy()


def _dev(t, dev, dtype=None):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.to(device=dev, dtype=dtype or t.dtype).contiguous()


def _float_roi(t, dev, what):
    t = _dev(t, dev)
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s: float32 or float64, not %s" % (what, t.dtype))
    return t


def compute_targets_batched(rois, gts_val, box_lbls, fg_thresh, ign_thresh, bg_thresh_lo, bg_thresh_hi, best_thresh, gts_ign=None,
                            val_counts=None, ign_counts=None, gts_3d=None, rois_3d=None, rois_3d_cen=None, anchors=None, anchor_cols=None,
                            tracker_col=4, means=None, stds=None, want=("transforms", "raw_gt", "ols_max", "best_roi"), out=None):
    """B images at once.  rois [B, R, >=4] (float32 / float64 device tensor; column tracker_col holds the anchor tracker when the 3D
    source is anchors[tracker]); gts_val [B, M, 4], box_lbls [B, M]; gts_ign [B, K, 4] or None; val_counts / ign_counts [B] (None: all
    M / K rows); gts_3d [B, M, D3] or None; rois_3d [B, R, >=8+] and rois_3d_cen [B, R, 2] (float32 / float64) or None; anchors [A, C]
    float64 or None; anchor_cols (default: anchors.shape[1], or 0 without anchors) sets decomp_alpha (>= 11) and has_vel (== 12).
    means / stds: the call site's bbox_means / bbox_stds (host), applied to transforms as rpn_3d.py:440-451 does, or None.
    want: the outputs to compute, among transforms, raw_gt, ols_max, ols, ols_ign, best_roi.  out: {name: tensor} to write into instead
    of new tensors (contiguous, of the output's shape and dtype).  Returns Targets (None where not wanted)."""
    lib = _lib.load()
    dev = rois.device if isinstance(rois, torch.Tensor) and rois.is_cuda else _device()
    rois = _float_roi(rois, dev, "rois")
    if rois.dim() != 3 or rois.shape[2] < 4:
        raise ValueError("rois must be [B, R, >=4], got %s" % (tuple(rois.shape),))
    B, R, ld = rois.shape
    gts_val = _dev(gts_val, dev, torch.float64)
    M = gts_val.shape[1] if gts_val is not None and gts_val.numel() else 0
    if M:
        gts_val = gts_val.reshape(B, M, 4)
    box_lbls = _dev(box_lbls, dev, torch.int32) if M else None
    if box_lbls is not None:
        box_lbls = box_lbls.reshape(B, M)
    gts_ign = _dev(gts_ign, dev, torch.float64)
    K = gts_ign.shape[1] if gts_ign is not None and gts_ign.numel() else 0
    if K:
        gts_ign = gts_ign.reshape(B, K, 4)
    vc = _dev(val_counts, dev, torch.int32)
    ic = _dev(ign_counts, dev, torch.int32)
    g3 = _dev(gts_3d, dev, torch.float64)
    if g3 is not None and (g3.dim() != 3 or g3.shape[0] != B or g3.shape[1] != M or g3.shape[2] == 0):
        raise ValueError("gts_3d must be [B, M, D3] = [%d, %d, D3], got %s" % (B, M, tuple(g3.shape)))
    D3 = g3.shape[2] if g3 is not None else 0            # sets the output widths, also when M = 0 (gts_3d is then empty)
    r3 = _float_roi(rois_3d, dev, "rois_3d") if rois_3d is not None else None
    cen = _float_roi(rois_3d_cen, dev, "rois_3d_cen") if rois_3d_cen is not None else None
    anc = _dev(anchors, dev, torch.float64) if anchors is not None and len(anchors) else None
    if anchor_cols is None:
        anchor_cols = anc.shape[1] if anc is not None else 0
    decomp = anchor_cols >= 11
    vel = anchor_cols == 12
    n_norm = 4 + ((9 if decomp else 7) if g3 is not None else 0)
    mh = _f64_host(means, n_norm, "means")
    sh = _f64_host(stds, n_norm, "stds")
    Wt = 5 + D3 + 2 * decomp + vel if g3 is not None else 5
    Wr = 5 + D3 if g3 is not None else 5

    given = out or {}

    def alloc(name, shape, dtype):
        if name not in want:
            return None
        t = given.get(name)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), dev))
        return t
    transforms = alloc("transforms", (B, R, Wt), torch.float32)
    raw_gt = alloc("raw_gt", (B, R, Wr), torch.float32)
    ols_max = alloc("ols_max", (B, R), torch.float64)
    ols = alloc("ols", (B, R, M), torch.float64) if M else None
    ols_ign = alloc("ols_ign", (B, R, K), torch.float64) if K else None
    best_roi = alloc("best_roi", (B, M), torch.int64)
    wsb = lib.gnms_compute_targets_workspace_bytes(B, R, M)
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    dp = lambda a: a.ctypes.data if a is not None else None          # noqa: E731
    with on_device(dev):
        rc = lib.gnms_compute_targets(
            ptr(rois), int(rois.dtype == torch.float64), B, R, ld, ptr(gts_val), ptr(box_lbls), M, ptr(vc), ptr(gts_ign), K, ptr(ic),
            ptr(g3), D3, ptr(r3), int(r3 is not None and r3.dtype == torch.float64), r3.shape[-1] if r3 is not None else 0,
            ptr(cen), int(cen is not None and cen.dtype == torch.float64), ptr(anc), anc.shape[0] if anc is not None else 0,
            int(anchor_cols), int(tracker_col), float(fg_thresh), float(ign_thresh), float(bg_thresh_lo), float(bg_thresh_hi),
            float(best_thresh), dp(mh), dp(sh), ptr(transforms), ptr(raw_gt), ptr(ols_max), ptr(ols), ptr(ols_ign), ptr(best_roi),
            ptr(ws), wsb, stream_ptr(dev))
    check(rc, "gnms_compute_targets")
    return Targets(transforms, raw_gt, ols_max, ols, ols_ign, best_roi)


def _np_rois(x):
    x = np.asarray(x)
    return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def compute_targets(gts_val, gts_ign, box_lbls, rois, fg_thresh, ign_thresh, bg_thresh_lo, bg_thresh_hi, best_thresh,
                    gts_3d=None, anchors=[], tracker=[], rois_3d=None, rois_3d_cen=None):
    """lib/rpn_util.py:411-524 on the GPU.  Returns (transforms float32 [R, W], ols float64 [R, M] or None when M = 0, raw_gt float32)."""
    rois = _np_rois(rois)
    R = rois.shape[0]
    gts_val = np.asarray(gts_val, dtype=np.float64).reshape(-1, 4)
    gts_ign = np.asarray(gts_ign, dtype=np.float64).reshape(-1, 4)
    M = gts_val.shape[0]
    anchors = None if anchors is None or len(anchors) == 0 else np.asarray(anchors, dtype=np.float64)
    has_3d = gts_3d is not None
    if has_3d:
        gts_3d = np.asarray(gts_3d, dtype=np.float64)
        if gts_3d.ndim != 2 or gts_3d.shape[0] != M:
            raise ValueError("gts_3d must be [M, D3] = [%d, D3], got %s" % (M, gts_3d.shape))
    # the rois as [R, 5]: x1 y1 x2 y2 and, where anchors[tracker] is the 3D source, int64(tracker) in column 4
    r5 = np.zeros((R, 5), dtype=rois.dtype)
    r5[:, :4] = rois[:, :4]
    use_tracker = has_3d and rois_3d is None and M > 0
    if use_tracker:
        r5[:, 4] = np.asarray(tracker).astype(np.int64)
    dev = _device()
    t = compute_targets_batched(
        torch.from_numpy(r5)[None].to(dev), torch.from_numpy(gts_val)[None].to(dev) if M else None,
        torch.from_numpy(np.asarray(box_lbls).astype(np.int32).reshape(1, M)).to(dev) if M else None,
        fg_thresh, ign_thresh, bg_thresh_lo, bg_thresh_hi, best_thresh,
        gts_ign=torch.from_numpy(gts_ign)[None].to(dev) if gts_ign.shape[0] else None,
        gts_3d=torch.from_numpy(gts_3d)[None].to(dev) if has_3d else None,
        rois_3d=torch.from_numpy(_np_rois(rois_3d))[None].to(dev) if rois_3d is not None and has_3d and M else None,
        rois_3d_cen=torch.from_numpy(_np_rois(rois_3d_cen))[None].to(dev) if rois_3d_cen is not None and has_3d and M else None,
        anchors=torch.from_numpy(anchors).to(dev) if use_tracker else None,
        anchor_cols=anchors.shape[1] if anchors is not None else 0, want=("transforms", "raw_gt", "ols"))
    ols = t.ols[0].cpu().numpy() if M else None
    return t.transforms[0].cpu().numpy(), ols, t.raw_gt[0].cpu().numpy()
