"""The RPN heads' maps -> the five tensors every entry behind the network takes (csrc/heads.hip): what the reference's
model does between its fifteen 1x1 convolutions and its return (models/densenet121_3d_dilate_decomp_alpha.py:166-245).

  assemble_heads   :166-215: the view / softmax / three sigmoids / fifteen flatten_tensor / two cat / clone chain, one launch forward
                   and one launch backward
  anchor_grid      :224-245: rois, rois_3d, rois_2d_cen, computed once on the host, uploaded once and cached, also as [B, R, .]

Layout: R = A * H * W, anchor row r = (a * H + h) * W + w -- the order of locate_anchors(..., convert_tensor=True) and of
view(B, C, A * H, W) + flatten_tensor.  cls_map [B, C * A, H, W] has channel c * A + a; the thirteen box maps [B, A, H, W] come in the
order of BOX_MAPS, axis and head before their sigmoid.  Device tensors in, device tensors out, nothing read back: both launches are
stream-ordered and can be captured in a graph with the loss behind them.  There is no CPU implementation here.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

__all__ = ["assemble_heads", "anchor_grid", "Heads", "BOX_MAPS"]

BOX_MAPS = ("x", "y", "w", "h", "x3d", "y3d", "z3d", "w3d", "h3d", "l3d", "alpha", "axis", "head")
N_MAPS = 15                                          # cls, BOX_MAPS, acceptance

Heads = collections.namedtuple("Heads", ["cls", "prob", "bbox_2d", "bbox_3d", "acceptance"])


def _block_contiguous(t):
    """the [., H, W] block of every image is contiguous (a dimension of size 1 may carry any stride)"""
    want = 1
    for d in (3, 2, 1):
        if t.shape[d] != 1 and t.stride(d) != want:
            return False
        want *= t.shape[d]
    return t.shape[0] == 1 or t.stride(0) >= 0


def _aligned_rows(g):
    """a cotangent as contiguous float32 rows on a 16-byte boundary (None stays None: the kernel takes it as zero)"""
    if g is None:
        return None
    g = g.to(torch.float32).contiguous()
    return g.clone() if g.data_ptr() % 16 else g


class _Assemble(torch.autograd.Function):
    """one launch forward, one launch backward; prob and the sigmoids are saved as the outputs they are"""

    @staticmethod
    def forward(ctx, *maps):
        ctx.set_materialize_grads(False)
        B, A, H, W = (int(v) for v in maps[1].shape)
        C = int(maps[0].shape[1]) // A
        R = A * H * W
        dev = maps[0].device
        src = []
        for t in maps:
            if t is not None:
                t = t.detach().to(torch.float32)
                if not _block_contiguous(t):
                    t = t.contiguous()
            src.append(t)
        c_maps = (ctypes.c_void_p * N_MAPS)(*[ptr(t) for t in src])
        c_strides = (ctypes.c_longlong * N_MAPS)(*[t.stride(0) if t is not None and B > 1 else 0 for t in src])
        cls = torch.empty((B, R, C), dtype=torch.float32, device=dev)
        prob = torch.empty((B, R, C), dtype=torch.float32, device=dev)
        bbox_2d = torch.empty((B, R, 4), dtype=torch.float32, device=dev)
        bbox_3d = torch.empty((B, R, 10), dtype=torch.float32, device=dev)
        acceptance = torch.empty((B, R, 1), dtype=torch.float32, device=dev) if src[-1] is not None else None
        lib = _lib.load()
        with _lib.on_device(dev):
            rc = lib.gnms_heads_assemble(ctypes.addressof(c_maps), ctypes.addressof(c_strides), B, A, H, W, C, ptr(cls), ptr(prob), ptr(bbox_2d),
                                         ptr(bbox_3d), ptr(acceptance), stream_ptr(dev))
        check(rc, "gnms_heads_assemble")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(prob, bbox_3d, acceptance)
            ctx.dims = (B, A, H, W, C)
            ctx.like = [(t.dtype, int(t.shape[1])) if t is not None else None for t in maps]
        return cls, prob, bbox_2d, bbox_3d, acceptance

    @staticmethod
    def backward(ctx, g_cls, g_prob, g_bbox_2d, g_bbox_3d, g_acceptance):
        prob, bbox_3d, acceptance = ctx.saved_tensors
        B, A, H, W, C = ctx.dims
        dev = prob.device
        cot = [_aligned_rows(g) for g in (g_cls, g_prob, g_bbox_2d, g_bbox_3d, g_acceptance)]
        grads = [torch.empty((B, like[1], H, W), dtype=torch.float32, device=dev) if like is not None and need else None
                 for like, need in zip(ctx.like, ctx.needs_input_grad)]
        c_grads = (ctypes.c_void_p * N_MAPS)(*[ptr(g) for g in grads])
        lib = _lib.load()
        with _lib.on_device(dev):
            rc = lib.gnms_heads_assemble_backward(ptr(prob), ptr(bbox_3d), ptr(acceptance), ptr(cot[0]), ptr(cot[1]), ptr(cot[2]), ptr(cot[3]),
                                                  ptr(cot[4]), B, A, H, W, C, ctypes.addressof(c_grads), stream_ptr(dev))
        check(rc, "gnms_heads_assemble_backward")
        return tuple(g.to(like[0]) if g is not None else None for g, like in zip(grads, ctx.like))


def assemble_heads(cls_map, box_maps, acceptance_map=None):
    """cls_map [B, C * A, H, W] (channel c * A + a), box_maps: the thirteen [B, A, H, W] maps in the order of BOX_MAPS (axis and head before
    their sigmoid), acceptance_map [B, A, H, W] or None (the "regress" head, before its sigmoid).  A map may be a channel slice of one
    stacked convolution output: it is read where it lies as long as its [., H, W] block is contiguous; anything else is copied first.
    Maps of another floating dtype are converted to float32 and get their gradient back in their own dtype.
    -> Heads(cls [B, R, C], prob [B, R, C], bbox_2d [B, R, 4], bbox_3d [B, R, 10], acceptance [B, R, 1] or None) with R = A * H * W and
    row r = (a * H + h) * W + w: float32, contiguous, freshly allocated, as the reference's model returns them and as sample_anchors,
    classification_loss, regression_loss, after_nms_loss and detections_from_heads take them.  bbox_3d is x3d y3d z3d w3d h3d l3d alpha
    alpha sigmoid(axis) sigmoid(head).  Differentiable w.r.t. all fifteen maps; the backward is one launch and reads prob, bbox_3d and
    acceptance as returned, so these three must not be modified in place before it (autograd checks); cls and bbox_2d may be -- the
    reference's bbox_transform_inv scales bbox_2d in place.  2 <= C <= 16, GnmsError outside."""
    box_maps = tuple(box_maps)
    if len(box_maps) != len(BOX_MAPS):
        raise ValueError("box_maps holds the %d maps %s, got %d" % (len(BOX_MAPS), " ".join(BOX_MAPS), len(box_maps)))
    maps = (cls_map,) + box_maps + (acceptance_map,)
    names = ("cls_map",) + BOX_MAPS + ("acceptance_map",)
    for name, t in zip(names, maps):
        if t is None and name == "acceptance_map":
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or not t.is_floating_point():
            raise ValueError("%s must be a 4-D floating tensor, got %s" % (name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    B, A, H, W = (int(v) for v in box_maps[0].shape)
    for name, t in zip(names[1:], maps[1:]):
        if t is not None and tuple(t.shape) != (B, A, H, W):
            raise ValueError("the box and acceptance maps must agree: %s is %s, x is %s" % (name, tuple(t.shape), (B, A, H, W)))
    if int(cls_map.shape[0]) != B or tuple(cls_map.shape[2:]) != (H, W):
        raise ValueError("cls_map must be [B, C * A, H, W] = [%d, C * %d, %d, %d], got %s" % (B, A, H, W, tuple(cls_map.shape)))
    if A < 1 or int(cls_map.shape[1]) % A:
        raise ValueError("cls_map has %d channels, no multiple of the %d anchors of the box maps" % (int(cls_map.shape[1]), A))
    dev = cls_map.device
    if dev.type != "cuda" or any(t is not None and t.device != dev for t in maps):
        raise ValueError("the maps must lie on one GPU (got %s); there is no CPU fallback" % ", ".join(sorted({str(t.device) for t in maps if t is not None})))
    return Heads(*_Assemble.apply(*maps))


GRID_CACHE_ENTRIES = 8                               # tables kept, least recently used dropped: image sizes that vary at inference must not pile up
_GRIDS = collections.OrderedDict()


def anchor_grid(anchors, feat_size, stride, batch=None, device=None):
    """The anchor tables of :224-245 for a feature map feat_size = (H, W): rois [R, 5] = x1 y1 x2 y2 anchor index, locate_anchors(anchors,
    feat_size, stride, convert_tensor=True) bit for bit (float64 on the host, then float32); rois_3d [R, anchors.shape[1]] =
    anchors[rois[:, 4]]; rois_2d_cen [R, 2] = the centres of :234-238 in float32 arithmetic.  Rows in the order of assemble_heads.
    With batch=B the three come back as contiguous [B, R, .] tensors, the stride pattern the loss entries read without a copy.  The
    tables are built and uploaded once per (anchors' contents, feat_size, stride, device, batch) and then shared between calls: treat
    them as read-only.  The GRID_CACHE_ENTRIES most recently used sets are kept, older ones dropped.  device=None: host tensors."""
    anchors = np.ascontiguousarray(np.asarray(anchors, dtype=np.float64))
    if anchors.ndim != 2 or anchors.shape[1] < 4:
        raise ValueError("anchors must be [A, >= 4], got %s" % (anchors.shape,))
    H, W = int(feat_size[0]), int(feat_size[1])
    dev = torch.device("cpu" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (anchors.tobytes(), anchors.shape, H, W, float(stride), str(dev))
    if (key, batch) in _GRIDS:
        _GRIDS.move_to_end((key, batch))
        return _GRIDS[(key, batch)]
    base = _GRIDS.get((key, None))
    if base is None:
        A = anchors.shape[0]
        xs = np.arange(W) * float(stride)                                   # rpn_util.py:980-991
        ys = np.arange(H) * float(stride)
        rois = np.empty((A, H, W, 5), np.float64)
        rois[..., 0] = xs[None, None, :] + anchors[:, 0, None, None]
        rois[..., 1] = ys[None, :, None] + anchors[:, 1, None, None]
        rois[..., 2] = xs[None, None, :] + anchors[:, 2, None, None]
        rois[..., 3] = ys[None, :, None] + anchors[:, 3, None, None]
        rois[..., 4] = np.arange(A, dtype=np.float64)[:, None, None]
        rois = torch.from_numpy(rois.reshape(-1, 5)).to(torch.float32)      # :227
        rois_3d = torch.from_numpy(anchors[rois[:, 4].long().numpy(), :]).to(torch.float32)     # :230-231
        widths = rois[:, 2] - rois[:, 0] + 1.0                              # :234-238, float32
        heights = rois[:, 3] - rois[:, 1] + 1.0
        cen = torch.stack((rois[:, 0] + 0.5 * widths, rois[:, 1] + 0.5 * heights), dim=1)
        base = _GRIDS[(key, None)] = tuple(t.to(dev).contiguous() for t in (rois, rois_3d, cen))
    got = base
    if batch is not None:
        B = int(batch)
        if B < 1:
            raise ValueError("batch must be >= 1, got %d" % B)
        got = _GRIDS[(key, batch)] = tuple(t.unsqueeze(0).expand(B, -1, -1).contiguous() for t in base)
    while len(_GRIDS) > GRID_CACHE_ENTRIES:                                # least recently used first; a caller's own reference keeps its tables alive
        _GRIDS.popitem(last=False)
    return got
