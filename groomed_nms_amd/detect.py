"""Inference post-processing of the detection head on the GPU (csrc/detect3d.hip): what the reference's lib/rpn_util.py::im_detect_3d
does between `net(im)` and the returned `aboxes` (:1087-1356), without its host round trip over every anchor.

  detections_from_heads   batched, device tensors in, a padded [B, Kmax, 14] tensor and counts [B] out; nothing leaves the device
  im_detect_3d            the reference's signature and return value (a float64 ndarray [n, 14]) on top of it, B = 1

Order of work: scores over all anchors -> top-K selection -> decode of the selected anchors only -> NMS -> assembly.
The reference decodes all ~127 k anchors, copies them to the host, sorts there and keeps 3000, then 500.
All arithmetic runs in HIP kernels behind the C ABI (include/groomed_nms_hip.h); no CPU implementation lives here.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, on_device

__all__ = ["detections_from_heads", "im_detect_3d", "camera_constants"]

_NMS = ("groomed", "classic", None)
_OVERLAPS = ("2d", "3d", "product")


def _device():
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _dev(x, dev, dtype):
    """a contiguous tensor of `dtype` on `dev` (NumPy / host data is uploaded: not inside a graph capture)"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    return x.detach().to(device=dev, dtype=dtype).contiguous()


def _norm(v, what):
    """bbox_means / bbox_stds ([1, n] or [n]) as a host float array: the kernels take them as arguments (rounded to fp32, as torch
    rounds the Python scalars of lib/rpn_util.py:1111-1128)"""
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    if a.size < 4:
        raise ValueError("%s needs at least 4 columns, got %d" % (what, a.size))
    a = a[:13].astype(np.float32)
    return (ctypes.c_float * a.size)(*a.tolist()), int(a.size)


def camera_constants(p2, scale_factor, im_hw, B, device=None):
    """The per-image constants of detections_from_heads as device tensors (p2_inv [B,4,4] float64, scale_factor [B] float32, im_hw [B,2]
    float32), for callers that build them once -- inside a graph capture nothing may be uploaded.  p2 [4,4] or [B,4,4] is inverted on the
    host in float64 (np.linalg.inv, lib/rpn_util.py:1069)."""
    dev = device if device is not None else _device()
    P = np.asarray(p2.detach().cpu().numpy() if isinstance(p2, torch.Tensor) else p2, dtype=np.float64)
    if P.shape[-2:] != (4, 4):
        raise ValueError("p2 must be [4, 4] or [B, 4, 4]")
    P = np.broadcast_to(P.reshape(-1, 4, 4), (B, 4, 4)) if P.size == 16 else P.reshape(-1, 4, 4)
    if P.shape[0] != B:
        raise ValueError("p2 holds %d matrices for %d images" % (P.shape[0], B))
    inv = np.stack([np.linalg.inv(P[b]) for b in range(B)])
    s = np.asarray(scale_factor.detach().cpu().numpy() if isinstance(scale_factor, torch.Tensor) else scale_factor, dtype=np.float64).reshape(-1)
    if s.size not in (1, B):
        raise ValueError("scale_factor must be a number or hold one per image")
    s = np.broadcast_to(s, (B,)).astype(np.float32)
    hw = np.asarray(im_hw.detach().cpu().numpy() if isinstance(im_hw, torch.Tensor) else im_hw, dtype=np.float64)
    if hw.shape[-1] != 2 or hw.size not in (2, 2 * B):
        raise ValueError("im_hw must be (height, width) or [B, 2]")
    hw = np.broadcast_to(hw.reshape(-1, 2), (B, 2)).astype(np.float32)
    return _dev(inv, dev, torch.float64), _dev(s, dev, torch.float32), _dev(hw, dev, torch.float32)


def _scores(prob, acceptance_prob=None):
    """gnms_detect3d_scores: prob [B,A,C], acceptance_prob [B,A] or [B,A,n] (column 0) -> (scores [B,A] fp32, cls_pred [B,A] int32)"""
    if not prob.is_cuda:
        raise _lib.GnmsError("detections_from_heads expects GPU tensors")
    if prob.dim() != 3 or prob.shape[2] < 2:
        raise ValueError("prob must be [B, A, C] with C >= 2")
    lib = _lib.load()
    dev = prob.device
    p = prob.detach().to(torch.float32).contiguous()
    B, A, C = p.shape
    acc, acc_ld = None, 1
    if acceptance_prob is not None:
        acc = acceptance_prob.detach().to(device=dev, dtype=torch.float32).contiguous()
        if acc.dim() not in (2, 3) or tuple(acc.shape[:2]) != (B, A) or (acc.dim() == 3 and acc.shape[2] < 1):
            raise ValueError("acceptance_prob must be [B, A] or [B, A, n]")
        acc_ld = acc.shape[2] if acc.dim() == 3 else 1
    scores = torch.empty((B, A), dtype=torch.float32, device=dev)
    cls_pred = torch.empty((B, A), dtype=torch.int32, device=dev)
    with on_device(dev):
        check(lib.gnms_detect3d_scores(ptr(p), ptr(acc), acc_ld, B, A, C, ptr(scores), ptr(cls_pred), stream_ptr(dev)), "gnms_detect3d_scores")
    return scores, cls_pred


def _decode(sel_index, K, bbox_2d, bbox_3d, rois, anchors, bbox_means, bbox_stds, p2_inv=None, scale_factor=None, counts=None,
                    decomp_alpha=True, want_raw=False):
    """gnms_detect3d_decode for the first K entries of sel_index [B, >=K] (int64, select_topk's output) -> (boxes2d [B,K,4], coords_3d
    [B,K,7], coords_3d_raw [B,K,7] or None).  Device tensors: bbox_2d [B,A,4], bbox_3d [B,A,D3], rois [A,5], anchors [n,cols] fp32, p2_inv
    [B,4,4] float64, scale_factor [B] fp32."""
    lib = _lib.load()
    dev = sel_index.device
    B, A = bbox_2d.shape[0], bbox_2d.shape[1]
    m, nm = _norm(bbox_means, "bbox_means")
    s, ns = _norm(bbox_stds, "bbox_stds")
    boxes2d = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    coords = torch.empty((B, K, 7), dtype=torch.float32, device=dev)
    raw = torch.empty((B, K, 7), dtype=torch.float32, device=dev) if want_raw else None
    with on_device(dev):
        check(lib.gnms_detect3d_decode(ptr(sel_index), sel_index.stride(0), ptr(counts), B, K, A, ptr(bbox_2d), ptr(bbox_3d), bbox_3d.shape[2],
                                       ptr(rois), ptr(anchors), anchors.shape[0], anchors.shape[1], m, s, min(nm, ns), int(bool(decomp_alpha)),
                                       ptr(p2_inv), ptr(scale_factor), ptr(boxes2d), ptr(coords), ptr(raw), stream_ptr(dev)),
              "gnms_detect3d_decode")
    return boxes2d, coords, raw


def _assemble(keep, keep_counts, sel_scores, sel_index, cls_pred, boxes2d, coords_3d, rois, clip_hw=None):
    """gnms_detect3d_assemble: keep [B, K] (int64 or int32 positions among the K decoded boxes; None: all of them in order) with
    keep_counts [B] -> (detections [B,K,14] fp32, counts [B] int32)"""
    lib = _lib.load()
    dev = boxes2d.device
    B, K = boxes2d.shape[0], boxes2d.shape[1]
    A = cls_pred.shape[1]
    out = torch.empty((B, K, 14), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    is64 = int(keep is not None and keep.dtype == torch.int64)
    if keep is not None and keep.dtype not in (torch.int64, torch.int32):
        raise ValueError("keep must be int64 or int32")
    with on_device(dev):
        check(lib.gnms_detect3d_assemble(ptr(keep), is64, keep.stride(0) if keep is not None else 0, ptr(keep_counts), ptr(sel_scores),
                                         sel_scores.stride(0), ptr(sel_index), sel_index.stride(0), ptr(cls_pred), ptr(boxes2d), ptr(coords_3d),
                                         ptr(rois), B, K, A, ptr(clip_hw), ptr(out), ptr(counts), stream_ptr(dev)), "gnms_detect3d_assemble")
    return out, counts


def _classic(boxes2d, nms_thres):
    """gnms_nms_sorted per image on the decoded boxes (sorted by score already): keep [B,K] int32, counts [B] int32"""
    lib = _lib.load()
    dev = boxes2d.device
    B, K = boxes2d.shape[0], boxes2d.shape[1]
    keep = torch.empty((B, K), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    nbytes = (max(int(lib.gnms_nms_workspace_bytes(K)), 256) + 255) // 256 * 256
    ws = torch.empty((B, nbytes), dtype=torch.uint8, device=dev)
    with on_device(dev):
        for b in range(B):
            check(lib.gnms_nms_sorted(ptr(boxes2d[b]), K, 4, float(nms_thres), ptr(keep[b]), ptr(counts[b:]), ptr(ws[b]), ws.shape[1],
                                      stream_ptr(dev)), "gnms_nms_sorted")
    return keep, counts


def detections_from_heads(prob, bbox_2d, bbox_3d, rois, anchors, bbox_means, bbox_stds, p2, scale_factor, im_hw, acceptance_prob=None, *,
                          nms="groomed", overlap_in_nms="2d", nms_thres=0.4, nms_topN_pre=3000, groomed_topN=500, decomp_alpha=True,
                          clip_boxes=False, pruning_method="linear", temperature=0.01, valid_box_prob_threshold=0.3, group_boxes=True,
                          mask_group_boxes=True, group_size=100, p2_inv=None, return_intermediates=False):
    """The detections of a batch of images from the network heads, on the device.

    prob [B,A,C] class probabilities (column 0 background), bbox_2d [B,A,4], bbox_3d [B,A,>=10] (>=7 without decomp_alpha), rois [A,5]
    (x1 y1 x2 y2 tracker), anchors [n,>=11] (rpn_conf.anchors), bbox_means / bbox_stds [1,13] (host), p2 [4,4] or [B,4,4], scale_factor a
    number or [B], im_hw (height, width) of the original image or [B,2], acceptance_prob [B,A(,1)] or None.
    nms: "groomed" (GrooMeD-NMS on the first `groomed_topN` of the `nms_topN_pre` best boxes, with `overlap_in_nms` in "2d" / "3d" /
    "product" and the layer's keyword set), "classic" (greedy NMS on all `nms_topN_pre`), or None (the `nms_topN_pre` best boxes as they
    are).  Returns (detections [B,Kmax,14] fp32 = x1 y1 x2 y2 score cls x y z w h l alpha tracker, rows behind the count zero; counts [B]
    int32), both on the device, in the reference's order (lib/rpn_util.py:1338-1351).

    Nothing is copied to the host and nothing waits for the device.  Host data among the arguments (p2, scale_factor, im_hw, NumPy
    anchors / rois) is uploaded first.

    Keywords beyond the reference's configuration:
      p2_inv=               the float64 inverse(s) [B,4,4] on the device, from camera_constants().  Then `p2` is not read (pass None) and
                            scale_factor / im_hw must be camera_constants()' device tensors too, one entry per image.  With these the
                            call is stream-ordered launches only and can be captured into a graph; the tests replay it at 768 anchors
                            and at 126 720 (where, under capture, gnms_select_topk runs its pre-selection with a stream-ordered
                            temporary instead of its cooperative launch).
      return_intermediates= also return a dict of the stages' device tensors (scores, cls_pred, sel_index, sel_scores, boxes2d,
                            coords_3d, coords_3d_raw, keep, keep_counts); coords_3d_raw is then computed for every route."""
    if nms not in _NMS:
        raise ValueError("nms must be one of %r" % (_NMS,))
    if overlap_in_nms not in _OVERLAPS:
        raise ValueError("overlap_in_nms must be one of %r" % (_OVERLAPS,))
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3 or prob.shape[2] < 2:
        raise ValueError("prob must be a [B, A, C] tensor with C >= 2")
    B, A = prob.shape[0], prob.shape[1]
    d3 = 10 if decomp_alpha else 7
    if tuple(bbox_2d.shape[:2]) != (B, A) or bbox_2d.dim() != 3 or bbox_2d.shape[2] != 4:
        raise ValueError("bbox_2d must be [B, A, 4]")
    if tuple(bbox_3d.shape[:2]) != (B, A) or bbox_3d.dim() != 3 or bbox_3d.shape[2] < d3:
        raise ValueError("bbox_3d must be [B, A, >=%d]" % d3)
    if rois.dim() != 2 or rois.shape[0] != A or rois.shape[1] < 5:
        raise ValueError("rois must be [A, 5]")
    if len(anchors.shape) != 2 or anchors.shape[1] < (11 if decomp_alpha else 9):
        raise ValueError("anchors must be [n, >=%d]" % (11 if decomp_alpha else 9))
    if int(nms_topN_pre) < 1 or int(groomed_topN) < 1:
        raise ValueError("nms_topN_pre and groomed_topN must be positive")
    if A == 0:
        raise ValueError("no anchors")
    if not prob.is_cuda:
        raise _lib.GnmsError("detections_from_heads expects GPU tensors; there is no CPU fallback")
    from . import proposals, overlaps, groomed_nms as G
    dev = prob.device
    b2 = bbox_2d.detach().to(device=dev, dtype=torch.float32).contiguous()
    b3 = bbox_3d.detach().to(device=dev, dtype=torch.float32).contiguous()
    r = _dev(rois, dev, torch.float32)
    r = r if r.shape[1] == 5 else r[:, :5].contiguous()
    an = _dev(anchors, dev, torch.float32)                              # :1132 .type(torch.cuda.FloatTensor)
    if p2_inv is None:
        p2_inv, sf, hw = camera_constants(p2, scale_factor, im_hw, B, dev)
    else:
        p2_inv = _dev(p2_inv, dev, torch.float64).reshape(-1, 4, 4)
        sf = _dev(scale_factor, dev, torch.float32).reshape(-1)
        hw = _dev(im_hw, dev, torch.float32).reshape(-1, 2)
        if p2_inv.shape[0] != B or sf.shape[0] != B or hw.shape[0] != B:
            raise ValueError("with p2_inv given, p2_inv / scale_factor / im_hw must hold one entry per image")
    # 1. the only pass over all anchors
    scores, cls_pred = _scores(prob, acceptance_prob)
    # 2. the nms_topN_pre best of them, sorted (:1260-1289)
    kpre = min(int(nms_topN_pre), A)
    sel_index, _, sel_scores, _ = proposals.select_topk(scores, kpre)
    # 3. decode of what the NMS will see
    K = min(kpre, int(groomed_topN)) if nms == "groomed" else kpre      # :1293-1294
    want_raw = (nms == "groomed" and overlap_in_nms != "2d") or return_intermediates
    boxes2d, coords, raw = _decode(sel_index, K, b2, b3, r, an, bbox_means, bbox_stds, p2_inv, sf, None, decomp_alpha, want_raw)
    # 4. the NMS
    if nms == "groomed":
        kw = dict(nms_threshold=nms_thres, pruning_method=pruning_method, temperature=temperature,
                  valid_box_prob_threshold=valid_box_prob_threshold, group_boxes=group_boxes, mask_group_boxes=mask_group_boxes,
                  group_size=group_size)
        s = sel_scores[:, :K].contiguous()
        if overlap_in_nms == "2d":                                      # :1295-1298
            out = G.differentiable_nms_with_iou2d_batched(s, boxes2d, **kw)
        else:                                                           # :1301-1317
            ov = overlaps.iou3d_batched(raw, from_params=True, nms_overlap=True, nms_threshold=nms_thres)
            if overlap_in_nms == "product":
                ov = overlaps.iou_batched(boxes2d) * ov
            out = G.differentiable_nms_batched(s, ov, **kw)
        keep, keep_counts = out[2], out[4]
    elif nms == "classic":                                              # :1334
        keep, keep_counts = _classic(boxes2d, nms_thres)
    else:
        keep, keep_counts = None, None
    # 5. the rows
    det, counts = _assemble(keep, keep_counts, sel_scores, sel_index, cls_pred, boxes2d, coords, r, hw if clip_boxes else None)
    if return_intermediates:
        return det, counts, dict(scores=scores, cls_pred=cls_pred, sel_index=sel_index, sel_scores=sel_scores, boxes2d=boxes2d, coords_3d=coords,
                                 coords_3d_raw=raw, keep=keep, keep_counts=keep_counts)
    return det, counts


def _conf(rpn_conf, key, default):
    return rpn_conf[key] if key in rpn_conf else default                # the reference's `default if not (key in conf) else conf.key`


def im_detect_3d(im, net, rpn_conf, preprocess, p2, gpu=0, synced=False, return_base=False):
    """
    Object detection in 3D -- lib/rpn_util.py:1052-1356, same arguments, same return value (float64 ndarray [n, 14]: x1 y1 x2 y2 score cls
    x y z w h l alpha tracker).  `preprocess` and `net` are called as the reference calls them; everything behind the network runs in
    detections_from_heads.  Branches no shipped configuration takes raise NotImplementedError.
    """
    use_differentiable_nms = _conf(rpn_conf, "use_nms_in_loss", False)                      # :1056-1063
    diff_nms_pruning_method = _conf(rpn_conf, "diff_nms_pruning_method", "linear")
    diff_nms_temperature = _conf(rpn_conf, "diff_nms_temperature", 1)
    diff_nms_valid_box_prob_threshold = _conf(rpn_conf, "diff_nms_valid_box_prob_threshold", 0.3)
    overlap_in_nms = _conf(rpn_conf, "overlap_in_nms", "2d")
    diff_nms_group_boxes = _conf(rpn_conf, "diff_nms_group_boxes", True)
    diff_nms_mask_group_boxes = _conf(rpn_conf, "diff_nms_mask_group_boxes", True)
    diff_nms_group_size = _conf(rpn_conf, "diff_nms_group_size", 100)
    if synced:
        raise NotImplementedError("im_detect_3d(synced=True) (the keep-column variant, lib/rpn_util.py:1268-1280) is not implemented")
    if return_base:
        raise NotImplementedError("im_detect_3d(return_base=True) is not implemented")
    if _conf(rpn_conf, "orientation_bins", 0) > 0:
        raise NotImplementedError("rpn_conf.orientation_bins > 0 (binned orientation head) is not implemented")
    if _conf(rpn_conf, "infer_2d_from_3d", False):
        raise NotImplementedError("rpn_conf.infer_2d_from_3d is not implemented")
    if _conf(rpn_conf, "has_un", False) or _conf(rpn_conf, "use_el_z", False):
        raise NotImplementedError("rpn_conf.has_un / rpn_conf.use_el_z (uncertainty columns) are not implemented")
    dev = torch.device("cuda", gpu) if torch.cuda.is_available() else None
    if dev is None:
        raise _lib.GnmsError("im_detect_3d needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    imH_orig = im.shape[0]
    imW_orig = im.shape[1]
    im = preprocess(im)
    if torch.is_tensor(im):                                                                 # preprocess.Preprocess: already on the device
        im = im[None].to(dev)
    else:
        im = torch.from_numpy(im[np.newaxis, :, :, :]).to(dev)                              # :1074
    imH = im.shape[2]
    scale_factor = imH / imH_orig                                                           # :1079
    cls, prob, bbox_2d, bbox_3d, feat_size, rois, acceptance_prob, acceptance_prob_cls = net(im)   # :1084
    acc = None
    if _conf(rpn_conf, "predict_acceptance_prob", False) and _conf(rpn_conf, "use_acceptance_prob_for_nms", False):   # :1253-1256
        acc = acceptance_prob[:1].to(dev)
    det, counts = detections_from_heads(
        prob[:1].to(dev), bbox_2d[:1].to(dev), bbox_3d[:1].to(dev), rois.to(dev), rpn_conf["anchors"], rpn_conf["bbox_means"], rpn_conf["bbox_stds"], p2,
        scale_factor, (imH_orig, imW_orig), acc, nms="groomed" if use_differentiable_nms else "classic", overlap_in_nms=overlap_in_nms,
        nms_thres=rpn_conf["nms_thres"], nms_topN_pre=rpn_conf["nms_topN_pre"], groomed_topN=500, decomp_alpha=bool(_conf(rpn_conf, "decomp_alpha", False)),
        clip_boxes=bool(rpn_conf["clip_boxes"]), pruning_method=diff_nms_pruning_method, temperature=diff_nms_temperature,
        valid_box_prob_threshold=diff_nms_valid_box_prob_threshold, group_boxes=diff_nms_group_boxes, mask_group_boxes=diff_nms_mask_group_boxes,
        group_size=diff_nms_group_size)
    n = int(counts[0])                                                                      # the one host read: the array's length
    return det[0, :n].cpu().numpy().astype(np.float64)
