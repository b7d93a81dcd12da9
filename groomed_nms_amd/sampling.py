"""Hard-anchor sampling, the sample weights and the weighted classification term of the RPN loss on the GPU (csrc/sampling.hip,
DESIGN.md 3.14): what lib/loss/rpn_3d.py does on the host between compute_targets and the NMS block.

  sample_anchors        :458-472 (labels), :583-612 (quotas, hard negatives, FG / BG encoding, bbox_weights), :885-887 (labels_scores)
  classification_loss   :893-907 (accuracy stats), :913-961 (weights, focal re-weighting), :976-1001 (the weighted term)
Device tensors in, device tensors out; nothing is read back and every launch is stream-ordered, so both calls can be captured in a
graph.  There is no CPU implementation here.  Ties among equal scores at a quota are resolved towards the lower anchor index (the
reference's np.argsort leaves them to the CPU's sort network).
"""
import collections
import math

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, on_device

__all__ = ["sample_anchors", "classification_loss", "Sample", "IGN_FLAG"]

IGN_FLAG = 3000            # GNMS_SAMPLE_IGN_FLAG


class Sample(collections.namedtuple("Sample", ["labels", "labels_scores", "bbox_weights", "fg_index", "fg_counts", "counts"])):
    """labels [B, R] int64 (0, class, IGN_FLAG); labels_scores [B, R] = prob[b, r, labels]; bbox_weights [B, R] (1 on the sampled
    foreground); fg_index [B, R] int32 with fg_counts [B]: the sampled foreground in ascending anchor order, -1 behind the count
    (proposals.select_topk's candidates / candidate_counts); counts [B, 6] int32 = n_fg, n_bg, fg_num, bg_num (the reference's
    quotas), sampled fg, sampled bg.  `sampled` [B, R] uint8 (0 no, 1 fg, 2 bg) is what classification_loss reads; it fills
    `labels_weight` [B, R]."""
    sampled = None
    labels_weight = None


def _device():
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def sample_anchors(target_labels, prob, val_counts, *, box_samples, fg_fraction, hard_negatives=True):
    """target_labels [B, R] float (Targets.transforms[..., 4]: > 0 the class, < 0 background, 0 ignore), prob [B, R, C], val_counts [B]
    (the valid ground truths per image as compute_targets_batched takes them; 0: the image is skipped, rpn_3d.py:406) or None.
    box_samples (float, math.inf: keep all) and fg_fraction (float or None) as in the reference's config.  Returns Sample."""
    if not hard_negatives:
        raise NotImplementedError("hard_negatives=False draws from NumPy's global RNG (lib/loss/rpn_3d.py:604-608); only the "
                                  "hard-negative sampler is implemented")
    box_samples = float(box_samples)
    if not math.isinf(box_samples) and fg_fraction is None:
        raise ValueError("a finite box_samples needs fg_fraction")
    lib = _lib.load()
    dev = prob.device if isinstance(prob, torch.Tensor) and prob.is_cuda else _device()
    p = prob.detach().to(device=dev, dtype=torch.float32).contiguous()
    if p.dim() != 3:
        raise ValueError("prob must be [B, R, C], got %s" % (tuple(p.shape),))
    B, R, C = p.shape
    t = target_labels.detach().to(device=dev, dtype=torch.float32)
    if tuple(t.shape) != (B, R):
        raise ValueError("target_labels must be [B, R] = [%d, %d], got %s" % (B, R, tuple(t.shape)))
    # a column of the targets rows is read where it lies: anchor stride ld, image stride R * ld
    if not (B == 0 or R == 0 or (t.stride(1) >= 1 and (B == 1 or t.stride(0) == R * t.stride(1)))):
        t = t.contiguous()
    ld = t.stride(1) if B and R else 1
    skip = None
    if val_counts is not None:
        skip = (torch.as_tensor(val_counts, device=dev).reshape(-1) <= 0).to(torch.uint8)
        if skip.numel() != B:
            raise ValueError("val_counts must be [B] = [%d]" % B)
    labels = torch.empty((B, R), dtype=torch.int64, device=dev)
    bbox_weights = torch.empty((B, R), dtype=torch.float32, device=dev)
    labels_scores = torch.empty((B, R), dtype=torch.float32, device=dev)
    sampled = torch.empty((B, R), dtype=torch.uint8, device=dev)
    fg_index = torch.empty((B, R), dtype=torch.int32, device=dev)
    fg_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 6), dtype=torch.int32, device=dev)
    wsb = lib.gnms_sample_anchors_workspace_bytes(B, R)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    with on_device(dev):
        rc = lib.gnms_sample_anchors(ptr(t), ld, ptr(p), ptr(skip), B, R, C, box_samples, int(fg_fraction is not None),
                                     float(fg_fraction) if fg_fraction is not None else 0.0, ptr(labels), ptr(bbox_weights),
                                     ptr(labels_scores), ptr(sampled), ptr(fg_index), ptr(fg_counts), ptr(counts), ptr(ws), wsb,
                                     stream_ptr(dev))
    check(rc, "gnms_sample_anchors")
    s = Sample(labels, labels_scores, bbox_weights, fg_index, fg_counts, counts)
    s.sampled = sampled
    return s


class _ClsLoss(torch.autograd.Function):
    """loss = the kernel's scalar; its gradient w.r.t. cls was written by the same call and is only scaled here"""

    @staticmethod
    def forward(ctx, cls, run):
        loss, dcls = run(cls.detach())
        ctx.save_for_backward(dcls)
        ctx.like = (cls.dtype, cls.shape)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (dcls,) = ctx.saved_tensors
        dtype, shape = ctx.like
        return (dcls * grad_output).to(dtype).reshape(shape), None


def _cls_term(cls, sample, *, fg_fraction, focal_loss=0, cls_2d_lambda=1):
    """classification_loss up to the launch -> (run, acc): run(x) launches gnms_cls_loss on the detached logits x and returns (loss [],
    dcls [B, R, C]); acc [2] float64 is filled by it.  Fills sample.labels_weight.  (Shared with loss.RPN_3D_loss, which scales dcls in
    its one backward launch.)"""
    lib = _lib.load()
    if sample.sampled is None:
        raise ValueError("sample must come from sample_anchors")
    dev = sample.labels.device
    B, R = sample.labels.shape
    if cls.dim() != 3 or cls.shape[0] != B or cls.shape[1] != R:
        raise ValueError("cls must be [B, R, C] = [%d, %d, C], got %s" % (B, R, tuple(cls.shape)))
    C = cls.shape[2]
    labels_weight = torch.empty((B, R), dtype=torch.float32, device=dev)
    acc = torch.empty((2,), dtype=torch.float64, device=dev)
    stat_counts = torch.empty((5,), dtype=torch.int32, device=dev)

    def run(x):
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dcls = torch.empty((B, R, C), dtype=torch.float32, device=dev)
        wsb = lib.gnms_cls_loss_workspace_bytes(B, R)
        ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
        with on_device(dev):
            rc = lib.gnms_cls_loss(ptr(x), ptr(sample.labels), ptr(sample.labels_scores), ptr(sample.sampled), ptr(sample.counts), B, R, C,
                                   int(fg_fraction is not None), float(fg_fraction) if fg_fraction is not None else 0.0,
                                   float(focal_loss), float(cls_2d_lambda), ptr(labels_weight), ptr(loss), ptr(dcls), ptr(acc),
                                   ptr(stat_counts), ptr(ws), wsb, stream_ptr(dev))
        check(rc, "gnms_cls_loss")
        return loss.reshape(()), dcls

    sample.labels_weight = labels_weight
    return run, acc


def classification_loss(cls, sample, *, fg_fraction, focal_loss=0, cls_2d_lambda=1):
    """cls [B, R, C] logits, sample from sample_anchors -> (loss, stats): loss a scalar tensor (differentiable w.r.t. cls), stats a
    dict of device scalars: acc_fg / acc_bg (float64; NaN when the batch has no such label) and cls (the term, detached).
    Fills sample.labels_weight."""
    run, acc = _cls_term(cls, sample, fg_fraction=fg_fraction, focal_loss=focal_loss, cls_2d_lambda=cls_2d_lambda)
    loss = _ClsLoss.apply(cls, run)
    return loss, {"acc_fg": acc[0], "acc_bg": acc[1], "cls": loss.detach()}
