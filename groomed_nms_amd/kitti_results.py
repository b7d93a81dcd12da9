"""The validation pass without result files: detections -> the rows the KITTI devkit would parse -> AP, on the device
(csrc/kitti_rows.hip, gnms_kitti_rows_append / gnms_round6).

The reference's tail (lib/train_test.py:99-110 -> lib/rpn_util.py:1489-1631 -> the devkit's fscanf) copies every image's boxes to the
host, back-projects them in NumPy, prints them with six decimals into one file per image and parses the files again.  What the
evaluation sees is a function of that text, so the kernels produce exactly the doubles the text parses to:

  round6        float64 device tensor -> float('{:.6f}'.format(v)) of every element
  KittiResults  collects a split: append() per batch (detections_from_heads' outputs; no host read, no synchronisation), finish()
                (the one host read) -> rows [n, 14] in kitti_eval's detection layout and det_offsets, evaluate() -> kitti_eval.evaluate,
                write() -> the reference's result files from the rounded rows (optional output)

There is no CPU implementation: host tensors raise GnmsError.  DESIGN.md 3.13.
"""
import os

import numpy as np
import torch

from . import _lib, kitti_eval
from ._lib import check, ptr, stream_ptr, on_device
from .kitti_io import _cfg

__all__ = ["round6", "KittiResults", "class_table", "MAX_LBLS"]

MAX_LBLS = 16                                                            # GNMS_KITTI_ROWS_MAX_LBLS
_STATE_WORDS = 8                                                         # GNMS_KITTI_ROWS_STATE_WORDS (int64)
_END, _IMAGES, _OUTSIDE, _ERRORS = 0, 1, 2, 3
_ERR_CLASS, _ERR_ANGLE = 1, 2
_ROW_FMT = "{} -1 -1" + " {:.6f}" * 13 + "\n"                            # lib/rpn_util.py:1626


def class_table(lbls):
    """conf.lbls -> the devkit's class id of every label (Car / Pedestrian / Cyclist -> 0 / 1 / 2 whatever the case, anything else -1)"""
    lbls = list(lbls)
    if not 1 <= len(lbls) <= MAX_LBLS:
        raise ValueError("lbls must name 1..%d classes, got %d" % (MAX_LBLS, len(lbls)))
    if not all(isinstance(s, str) and s and not any(c.isspace() for c in s) for s in lbls):
        raise ValueError("lbls must be non-empty strings without white space")
    return np.array([kitti_eval._det_class(s) for s in lbls], np.int32)


def _cuda_device(device):
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.GnmsError("device must be a GPU; there is no CPU fallback")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def round6(x, count=None):
    """The doubles that the 6-decimal text of x's elements parses to: float('{:.6f}'.format(v)), element for element, signed zeros
    included.  x: a float64 device tensor.  Exact for finite |v| < 1e9; other elements are returned as they are, and `count` (an int64
    device tensor with one element, optional) is incremented once for each of them."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64:
        raise ValueError("round6 expects a float64 tensor")
    if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int64 or count.numel() != 1):
        raise ValueError("count must be an int64 tensor with one element")
    if not x.is_cuda or (count is not None and count.device != x.device):
        raise _lib.GnmsError("round6 expects GPU tensors; there is no CPU fallback")
    lib = _lib.load()
    src = x.detach().contiguous()
    out = torch.empty_like(src)
    with on_device(x.device):
        check(lib.gnms_round6(ptr(src), ptr(out), src.numel(), ptr(count), stream_ptr(x.device)), "gnms_round6")
    return out


class KittiResults:
    """The detections of a split as the rows the devkit would read from the reference's result files, collected on the device.

    lbls           conf.lbls: label k + 1 of the detections' cls column is lbls[k]
    score_thres    conf.score_thres: a box is kept when its score, widened to float64, is > score_thres
    nms_topN_post  conf.nms_topN_post: only the first so many boxes of an image take part
    max_images     images the accumulator has room for
    capacity_rows  rows it has room for (at most max_images * nms_topN_post are ever needed)
    """

    def __init__(self, lbls, score_thres, nms_topN_post, max_images, capacity_rows, device=None):
        self.lbls = list(lbls)
        class_ids = class_table(self.lbls)
        self.score_thres = float(score_thres)
        if self.score_thres != self.score_thres:
            raise ValueError("score_thres is NaN")
        self.nms_topN_post = int(nms_topN_post)
        self.max_images, self.capacity_rows = int(max_images), int(capacity_rows)
        if self.nms_topN_post < 0 or self.max_images < 0 or self.capacity_rows < 0:
            raise ValueError("nms_topN_post, max_images and capacity_rows must not be negative")
        if self.max_images >= 2 ** 31 - 1 or self.capacity_rows >= 2 ** 31:
            raise ValueError("max_images / capacity_rows out of the int32 range")
        dev = self.device = _cuda_device(device)
        _lib.load()
        self._class_ids = torch.from_numpy(class_ids).to(dev)
        self._rows = torch.empty((self.capacity_rows, kitti_eval.DET_COLS), dtype=torch.float64, device=dev)
        self._lbl_index = torch.empty((self.capacity_rows,), dtype=torch.int32, device=dev)
        # the status words (int64) and the offsets (int32) share one buffer: finish() reads it with one copy
        self._meta = torch.zeros((2 * _STATE_WORDS + self.max_images + 1,), dtype=torch.int32, device=dev)
        self._state = self._meta[:2 * _STATE_WORDS].view(torch.int64)
        self._offsets = self._meta[2 * _STATE_WORDS:]
        self.n_images = 0                                                # known on the host: the batch sizes
        self.nonfinite_fields = None                                     # set by finish()
        self.unwrapped_angles = None

    @classmethod
    def from_conf(cls, conf, max_images, capacity_rows=None, device=None):
        """from the reference's configuration (lbls, score_thres, nms_topN_post); capacity_rows defaults to max_images * nms_topN_post"""
        if _cfg(conf, "has_un") or _cfg(conf, "use_un_for_score"):
            raise NotImplementedError("conf.has_un / conf.use_un_for_score (uncertainty-weighted scores) are not implemented")
        topn = int(_cfg(conf, "nms_topN_post"))
        cap = int(max_images) * topn if capacity_rows is None else capacity_rows
        return cls(_cfg(conf, "lbls"), _cfg(conf, "score_thres"), topn, max_images, cap, device=device)

    def append(self, det, counts, p2_inv):
        """One batch, in image order: det [B, Kmax, 14] fp32 and counts [B] int32 (detections_from_heads' outputs), p2_inv [B, 4, 4]
        float64 (camera_constants').  Stream-ordered kernel launches only: nothing is read on the host and nothing waits."""
        for t, what in ((det, "det"), (counts, "counts"), (p2_inv, "p2_inv")):
            if not isinstance(t, torch.Tensor):
                raise ValueError("%s must be a tensor" % what)
        if det.dim() != 3 or det.shape[2] != 14 or det.dtype != torch.float32:
            raise ValueError("det must be a float32 [B, Kmax, 14] tensor")
        B, Kmax = det.shape[0], det.shape[1]
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
            raise ValueError("counts must be an int32 [B] tensor")
        if p2_inv.dtype != torch.float64 or tuple(p2_inv.shape) != (B, 4, 4):
            raise ValueError("p2_inv must be a float64 [B, 4, 4] tensor")
        if B * Kmax >= 2 ** 31 or self.n_images + B >= 2 ** 31 - 1:
            raise ValueError("batch too large")
        dev = self.device
        if not (det.is_cuda and counts.is_cuda and p2_inv.is_cuda):
            raise _lib.GnmsError("KittiResults.append expects GPU tensors; there is no CPU fallback")
        if det.device != dev or counts.device != dev or p2_inv.device != dev:
            raise ValueError("the batch lives on another device than the accumulator (%s)" % dev)
        lib = _lib.load()
        det, counts, p2_inv = det.detach().contiguous(), counts.contiguous(), p2_inv.contiguous()
        scratch = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
        with on_device(dev):
            check(lib.gnms_kitti_rows_append(ptr(det), 14, ptr(counts), ptr(p2_inv), B, Kmax, self.nms_topN_post, self.score_thres,
                                             ptr(self._class_ids), len(self.lbls), ptr(scratch), ptr(self._rows), ptr(self._lbl_index),
                                             self.capacity_rows, ptr(self._offsets), self.max_images + 1, self.n_images, ptr(self._state),
                                             stream_ptr(dev)), "gnms_kitti_rows_append")
        self.n_images += B

    def finish(self):
        """(rows [n, 14] float64 on the device, det_offsets [I + 1] np.int32) of everything appended so far -- the one host read (the
        status words and the offsets, in one copy).  Raises ValueError when more rows were needed than capacity_rows, more images were
        appended than max_images, or a class index lay outside lbls.  Sets nonfinite_fields (fields that are not finite or not below 1e9
        in magnitude: stored as they are) and unwrapped_angles."""
        meta = self._meta.cpu().numpy()
        state = meta[:2 * _STATE_WORDS].view(np.int64)
        rows_needed, images_needed = int(state[_END]), int(state[_IMAGES])
        if images_needed > self.max_images:
            raise ValueError("%d images were appended, max_images is %d" % (images_needed, self.max_images))
        if rows_needed > self.capacity_rows:
            raise ValueError("%d rows were needed, capacity_rows is %d" % (rows_needed, self.capacity_rows))
        if int(state[_ERRORS]) & _ERR_CLASS:
            raise ValueError("a detection's class index lies outside lbls (%d labels)" % len(self.lbls))
        self.nonfinite_fields = int(state[_OUTSIDE])
        self.unwrapped_angles = bool(int(state[_ERRORS]) & _ERR_ANGLE)
        offsets = meta[2 * _STATE_WORDS:2 * _STATE_WORDS + images_needed + 1].copy()
        return self._rows[:rows_needed], offsets

    def evaluate(self, gt, gt_offsets, variants=(kitti_eval.MAIN,)):
        """finish() + kitti_eval.evaluate: one dict per variant"""
        rows, offsets = self.finish()
        return kitti_eval.evaluate(rows, offsets, gt, gt_offsets, variants=variants, device=self.device)

    def write(self, folder, ids):
        """<folder>/<id>.txt for every image, the bytes kitti_io.write_image_boxes_to_txt_file writes for the same boxes: host formatting
        of the device rows (printing a rounded value with six decimals reproduces its digits).  Returns the texts."""
        rows, offsets = self.finish()
        ids = list(ids)
        if len(ids) != offsets.size - 1:
            raise ValueError("%d ids for %d images" % (len(ids), offsets.size - 1))
        rows_h = rows.cpu().numpy()
        lbl_h = self._lbl_index[:rows_h.shape[0]].cpu().numpy()
        texts = []
        for i, name in enumerate(ids):
            text = "".join(_ROW_FMT.format(self.lbls[lbl_h[k]], *rows_h[k, 1:].tolist()) for k in range(offsets[i], offsets[i + 1]))
            with open(os.path.join(folder, str(name) + ".txt"), "w") as f:
                f.write(text)
            texts.append(text)
        return texts
