"""The two calls the reference makes before its first training step (scripts/train_rpn_3d.py:76-79), with their signatures and side
effects: what turns a config and an imdb into `conf.anchors`, `conf.bbox_means` and `conf.bbox_stds`.

  generate_anchors     lib/rpn_util.py:24-216: the 2D anchors from anchor_scales x anchor_ratios and, with has_3d, the per-anchor means of
                       the ground truths each anchor attracts.  On the HOST, on purpose: a few dozen anchors against a few thousand
                       ground truths, once per data set (as kitti_io.py is host code), with the reference's NumPy calls in the
                       reference's order, so the result is the reference's bit for bit (float32 2D columns widened to float64 at :97).
  compute_bbox_stats   lib/rpn_util.py:547-736 on the GPU: per image gnms_gt_filter (determine_ignores + bbXYWH2Coords; use_trunc in
                       the mean pass only, :594 against :668) -> gnms_compute_targets with the raw transforms (float64 rois,
                       anchors[tracker] as the 3D source) -> gnms_bbox_stats_partials, and one gnms_bbox_stats_finish per pass
                       (csrc/bbox_stats.hip).  The images are grouped by feat_size and batched within a group; the per-image partials
                       lie at the image's position in the imdb and are reduced in that order, so neither grouping, batch size nor visit
                       order changes a bit of the result.  Nothing is read back before the end of the second pass.

`cache_folder` behaves as in the reference: anchors.pkl / bbox_means.pkl + bbox_stds.pkl are read when they exist and written otherwise,
plain pickles of the ndarrays (lib/util.py:233-248), so a folder is interchangeable with the reference's.

Supported: has_3d=True, decomp_alpha=True, cluster_anchors 0 or absent, no has_vel; anything else raises NotImplementedError naming the
key.  `imdb`: a sequence of objects with gts, scale, imH, imW; a ground truth has cls, ign, visibility, trunc, bbox_full [4], bbox_3d
[>= 16]; attribute or key access, as in loss.pack_ground_truths.  More than 256 ground truths in an image: ValueError.
There is no CPU implementation of compute_bbox_stats here.
"""
import collections
import logging
import os
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .loss import RECORD_COLS, MAX_GTS, _field
from . import targets

__all__ = ["generate_anchors", "compute_bbox_stats", "pack_records", "group_by_feat_size", "image_partials", "sequential_f32_sum", "COLUMNS",
           "STAT_COLS", "PackedImdb", "Partials"]

STAT_COLS = 13                                       # GNMS_BBOX_STATS_COLS: transforms[:, 0:4] and transforms[:, 5:14]
COLUMNS = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13)  # of compute_targets' transforms; column 4 is the label
TRANSFORM_COLS = 5 + 16 + 2                          # compute_targets' transforms with bbox_3d [16] and decomp_alpha (:431)
DEFAULT_BATCH = 16                                   # images per launch: B * R rows of float64 rois and float32 transforms are held

PackedImdb = collections.namedtuple("PackedImdb", ["records", "counts", "feat_sizes", "scale_factors"])
Partials = collections.namedtuple("Partials", ["sums", "sq_sums", "counts", "used"])


def _has(conf, key):
    return key in conf and bool(conf[key])


def _check_conf(conf, who):
    for key, bad in (("has_3d", not _has(conf, "has_3d")), ("decomp_alpha", not _has(conf, "decomp_alpha")),
                     ("cluster_anchors", _has(conf, "cluster_anchors")), ("has_vel", _has(conf, "has_vel"))):
        if bad:
            raise NotImplementedError("%s: %s=%r is not implemented (supported: has_3d, decomp_alpha, no cluster_anchors, no has_vel)"
                                      % (who, key, conf[key] if key in conf else None))


def _pickle_read(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _pickle_write(path, obj):
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def _scale_factor(conf, imobj):
    return _field(imobj, "scale") * conf["test_scale"] / _field(imobj, "imH")          # :69, :589


# ------------------------------------------------------------------------------------------------ generate_anchors (host)
def anchor_center(w, h, stride):
    """:219-235"""
    anchor = np.zeros([4], dtype=np.float32)
    anchor[0] = -w / 2 + (stride - 1) / 2
    anchor[1] = -h / 2 + (stride - 1) / 2
    anchor[2] = w / 2 + (stride - 1) / 2
    anchor[3] = h / 2 + (stride - 1) / 2
    return anchor


def _ignores(gts, lbls, ilbls, min_gt_vis, min_gt_h, max_gt_h, scale_factor, use_trunc=False):
    """determine_ignores, :937-962"""
    igns = np.zeros([len(gts)], dtype=bool)
    rmvs = np.zeros([len(gts)], dtype=bool)
    both = list(lbls) + list(ilbls)
    for gtind, gt in enumerate(gts):
        ign = bool(_field(gt, "ign", False))
        ign |= bool(_field(gt, "visibility", 1.0) < min_gt_vis)
        ign |= bool(_field(gt, "bbox_full")[3] * scale_factor < min_gt_h)
        ign |= bool(_field(gt, "bbox_full")[3] * scale_factor > max_gt_h)
        ign |= _field(gt, "cls") in ilbls
        if use_trunc:
            ign |= bool(_field(gt, "trunc", 0.0) > max(1 - min_gt_vis, 0))
        igns[gtind] = ign
        rmvs[gtind] = _field(gt, "cls") not in both
    return igns, rmvs


def _xywh_to_coords(box):
    """bbXYWH2Coords, :781-791"""
    if box.shape[0] == 0:
        return np.empty([0, 4], dtype=float)
    box[:, 2] += box[:, 0] - 1
    box[:, 3] += box[:, 1] - 1
    return box


def _iou(box_a, box_b):
    """lib/core.py:480-513 (and intersect, :205-218), the NumPy 'combinations' branch"""
    max_xy = np.minimum(box_a[:, 2:4], np.expand_dims(box_b[:, 2:4], axis=1))
    min_xy = np.maximum(box_a[:, 0:2], np.expand_dims(box_b[:, 0:2], axis=1))
    inter = np.clip((max_xy - min_xy), a_min=0, a_max=None)
    inter = inter[:, :, 0] * inter[:, :, 1]
    area_a = ((box_a[:, 2] - box_a[:, 0]) * (box_a[:, 3] - box_a[:, 1]))
    area_b = ((box_b[:, 2] - box_b[:, 0]) * (box_b[:, 3] - box_b[:, 1]))
    union = np.expand_dims(area_a, 0) + np.expand_dims(area_b, 1) - inter
    return (inter / union).T


def generate_anchors(conf, imdb, cache_folder=None):
    """lib/rpn_util.py:24-216: sets conf.anchors ([A, 11] float64; anchors no ground truth is assigned to are dropped).  Host NumPy."""
    _check_conf(conf, "generate_anchors")
    if (cache_folder is not None) and os.path.exists(os.path.join(cache_folder, "anchors.pkl")):
        conf["anchors"] = _pickle_read(os.path.join(cache_folder, "anchors.pkl"))
        return
    stride = conf["feat_stride"]
    anchors = np.zeros([len(conf["anchor_scales"]) * len(conf["anchor_ratios"]), 4], dtype=np.float32)
    aind = 0
    for scale in conf["anchor_scales"]:                                                # :46-54
        for ratio in conf["anchor_ratios"]:
            h = scale
            w = scale * ratio
            anchors[aind, 0:4] = anchor_center(w, h, stride)
            aind += 1
    normalized_gts = None
    for imobj in imdb:                                                                 # :64-94
        gts = _field(imobj, "gts")
        if len(gts) > MAX_GTS:
            raise ValueError("an image has %d ground truths, %d are supported" % (len(gts), MAX_GTS))
        if len(gts) > 0:
            scale = _scale_factor(conf, imobj)
            igns, rmvs = _ignores(gts, conf["lbls"], conf["ilbls"], conf["min_gt_vis"], conf["min_gt_h"], np.inf, scale)
            keep = (rmvs == False) & (igns == False)                                   # noqa: E712
            gts_all = _xywh_to_coords(np.array([np.asarray(_field(gt, "bbox_full")) * scale for gt in gts]))
            gts_val = gts_all[keep, :]
            gts_3d = np.array([np.asarray(_field(gt, "bbox_3d")) for gt in gts])
            gts_3d = gts_3d[keep, :]
            for gtind in range(0, gts_val.shape[0]):
                w = gts_val[gtind, 2] - gts_val[gtind, 0] + 1
                h = gts_val[gtind, 3] - gts_val[gtind, 1] + 1
                gts_val[gtind, 0:4] = anchor_center(w, h, stride)
            if gts_val.shape[0] > 0:
                gt_info = np.ones([gts_val.shape[0], 100]) * -1
                gt_info[:, :(gts_val.shape[1] + gts_3d.shape[1])] = np.concatenate((gts_val, gts_3d), axis=1)
                normalized_gts = gt_info if normalized_gts is None else np.vstack((normalized_gts, gt_info))
    if normalized_gts is None:
        raise ValueError("generate_anchors: the imdb has no valid ground truth (the reference fails here as well)")
    anchors = np.concatenate((anchors, np.zeros([anchors.shape[0], 5])), axis=1)      # :97: float64 from here on
    anchors = np.concatenate((anchors, np.zeros([anchors.shape[0], 2])), axis=1)      # :100, decomp_alpha
    cols = (6, 7, 8, 9, 10, 16, 17)                                                    # z3d w3d h3d l3d rotY sin cos of the gt_info row
    lists = [[[] for _ in cols] for _ in range(anchors.shape[0])]
    ols = _iou(anchors[:, 0:4], normalized_gts[:, 0:4])                                # :119-121
    gt_target_ols = np.amax(ols, axis=0)
    gt_target_anchor = np.argmax(ols, axis=0)
    for gtind, gt in enumerate(normalized_gts):                                        # :124-138
        if gt_target_ols[gtind] > 0.2:
            for k, c in enumerate(cols):
                lists[gt_target_anchor[gtind]][k].append(gt[c])
    for aind in range(0, anchors.shape[0]):                                            # :157-190
        if len(lists[aind][0]) > 0:
            for k in range(len(cols)):
                anchors[aind, 4 + k] = np.mean(np.array(lists[aind][k]))
        else:
            logging.info("WARNING: Non-used anchor #{} found. Removing this anchor.".format(aind))
            anchors[aind, :] = -1
    anchors = anchors[np.all(anchors == -1, axis=1) == False, :]                       # noqa: E712  (:193)
    if cache_folder is not None:
        _pickle_write(os.path.join(cache_folder, "anchors.pkl"), anchors)
    conf["anchors"] = anchors


# ------------------------------------------------------------------------------------------------ compute_bbox_stats (device)
def pack_records(conf, imdb):
    """The imdb as the records gnms_gt_filter reads (loss.RECORD_COLS float64 per ground truth), with the reference's scaling done here
    in float64 by the same NumPy products (:598, :617, :950): bbox_full * scale_factor and bbox_3d[0:2] * scale_factor, so that the
    filter at its scale of 1 reproduces determine_ignores and bbXYWH2Coords exactly.  -> PackedImdb(records [N, cap, RECORD_COLS],
    counts [N] int32, feat_sizes [N, 2] (:590), scale_factors [N]); cap = the most ground truths of an image (>= 1)."""
    N = len(imdb)
    most = max([len(_field(im, "gts")) for im in imdb] + [1])
    if most > MAX_GTS:
        raise ValueError("an image has %d ground truths, %d are supported" % (most, MAX_GTS))
    ids = {name: 1.0 + i for i, name in enumerate(conf["lbls"])}
    ids.update({name: 0.0 for name in conf["ilbls"]})
    rec = np.zeros((N, most, RECORD_COLS), np.float64)
    counts = np.zeros((N,), np.int32)
    feat = np.zeros((N, 2), np.int64)
    scales = np.zeros((N,), np.float64)
    for i, imobj in enumerate(imdb):
        gts = _field(imobj, "gts")
        scale_factor = _scale_factor(conf, imobj)
        scales[i] = scale_factor
        feat[i] = np.ceil(np.array(np.array([_field(imobj, "imH"), _field(imobj, "imW")]) * scale_factor) / conf["feat_stride"]).astype(int)
        counts[i] = len(gts)
        for j, g in enumerate(gts):
            row = rec[i, j]
            row[0:4] = (np.asarray(_field(g, "bbox_full")) * scale_factor)[:4]
            b3 = np.array(np.asarray(_field(g, "bbox_3d"), np.float64).reshape(-1)[:16])
            b3[0:2] *= scale_factor
            row[4:4 + len(b3)] = b3
            row[20] = ids.get(_field(g, "cls"), -1.0)
            row[21] = 1.0 if _field(g, "ign", False) else 0.0
            row[22] = _field(g, "visibility", 1.0)
            row[23] = _field(g, "trunc", 0.0)
    return PackedImdb(rec, counts, feat, scales)


def group_by_feat_size(packed, visit_order=None):
    """{(H, W): [image indices]} of the images WITH ground truths (:587), in the order they are visited (default: imdb order)."""
    order = range(len(packed.counts)) if visit_order is None else visit_order
    groups = collections.OrderedDict()
    for i in order:
        if packed.counts[i] > 0:
            groups.setdefault((int(packed.feat_sizes[i, 0]), int(packed.feat_sizes[i, 1])), []).append(int(i))
    return groups


def _rois_f64(anchors, feat_size, stride):
    """locate_anchors(anchors, feat_size, stride) with convert_tensor=False (:965-1034): float64 [R, 5], row (a * H + h) * W + w"""
    A = anchors.shape[0]
    H, W = feat_size
    xs = np.array(range(0, W, 1)) * float(stride)
    ys = np.array(range(0, H, 1)) * float(stride)
    rois = np.empty((A, H, W, 5), np.float64)
    rois[..., 0] = xs[None, None, :] + anchors[:, 0, None, None]
    rois[..., 1] = ys[None, :, None] + anchors[:, 1, None, None]
    rois[..., 2] = xs[None, None, :] + anchors[:, 2, None, None]
    rois[..., 3] = ys[None, :, None] + anchors[:, 3, None, None]
    rois[..., 4] = np.arange(A, dtype=np.float64)[:, None, None]
    return rois.reshape(-1, 5)


def sequential_f32_sum(rows):
    """np.sum(rows, axis=0) of a C-contiguous float32 [m, k] array as the device adds it: from +0, one float32 addition per row in row
    order (tests/test_bbox_stats_host.py holds it to np.sum bit for bit)."""
    rows = np.asarray(rows, np.float32)
    acc = np.zeros((rows.shape[1],), np.float32)
    for i in range(rows.shape[0]):
        acc = (acc + rows[i]).astype(np.float32)
    return acc


class _Pass:
    """the device state both passes share: records, per-image partials, and the tables of each feat_size"""

    def __init__(self, conf, packed, dev):
        self.conf, self.packed, self.dev = conf, packed, dev
        self.lib = _lib.load()
        self.N, self.cap = packed.records.shape[0], packed.records.shape[1]
        self.records = torch.from_numpy(packed.records).to(dev)
        self.counts = torch.from_numpy(packed.counts).to(dev)
        self.used = torch.from_numpy((packed.counts > 0).astype(np.uint8)).to(dev)
        self.anchors = np.ascontiguousarray(np.asarray(conf["anchors"], np.float64))
        if self.anchors.ndim != 2 or self.anchors.shape[1] != 11:
            raise ValueError("conf.anchors must be [A, 11] (decomp_alpha), got %s" % (self.anchors.shape,))
        self.anchors_dev = torch.from_numpy(self.anchors).to(dev)
        self.rois = {}

    def run(self, use_trunc, means, batch_size, visit_order):
        """one pass over the imdb -> (sums float32 [N, 13] or sq_sums float64 [N, 13], counts int32 [N]) on the device"""
        conf, dev, lib, N, cap = self.conf, self.dev, self.lib, self.N, self.cap
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        sums = torch.empty((N, STAT_COLS), dtype=torch.float32, device=dev) if means is None else None
        sq = torch.empty((N, STAT_COLS), **f64) if means is not None else None
        fg = torch.empty((N,), **i32)
        st = stream_ptr(dev)
        for feat_size, images in group_by_feat_size(self.packed, visit_order).items():
            if feat_size not in self.rois:
                self.rois[feat_size] = torch.from_numpy(_rois_f64(self.anchors, feat_size, conf["feat_stride"])).to(dev)
            rois1 = self.rois[feat_size]
            R = rois1.shape[0]
            step = len(images) if not batch_size else int(batch_size)
            bufs = {}
            for lo in range(0, len(images), step):
                ids = torch.tensor(images[lo:lo + step], dtype=torch.int64).to(dev)
                B = ids.numel()
                if B not in bufs:
                    bufs[B] = (rois1.unsqueeze(0).expand(B, -1, -1).contiguous(), torch.empty((B, R, TRANSFORM_COLS), dtype=torch.float32, device=dev))
                rois, transforms = bufs[B]
                rec, cnt = self.records.index_select(0, ids), self.counts.index_select(0, ids)
                gts_val, gts_ign = torch.empty((B, cap, 4), **f64), torch.empty((B, cap, 4), **f64)
                gts_3d, box_lbls = torch.empty((B, cap, 16), **f64), torch.empty((B, cap), **i32)
                val_counts, ign_counts = torch.empty((B,), **i32), torch.empty((B,), **i32)
                with _lib.on_device(dev):              # :594-617; max_gt_h = inf, the scaling is in the records
                    check(lib.gnms_gt_filter(ptr(rec), ptr(cnt), B, cap, float(conf["min_gt_vis"]), float(conf["min_gt_h"]), float("inf"),
                                             int(bool(use_trunc)), ptr(gts_val), ptr(box_lbls), ptr(gts_3d), ptr(gts_ign), ptr(val_counts),
                                             ptr(ign_counts), st), "gnms_gt_filter")
                targets.compute_targets_batched(rois, gts_val, box_lbls, conf["fg_thresh"], conf["ign_thresh"], conf["bg_thresh_lo"],
                                                conf["bg_thresh_hi"], conf["best_thresh"], gts_ign=gts_ign, val_counts=val_counts,
                                                ign_counts=ign_counts, gts_3d=gts_3d, anchors=self.anchors_dev, tracker_col=4,
                                                want=("transforms",), out={"transforms": transforms})           # :620-622
                ids32 = ids.to(torch.int32)
                with _lib.on_device(dev):              # :629-650 / :702-713
                    check(lib.gnms_bbox_stats_partials(ptr(transforms), B, R, TRANSFORM_COLS, ptr(ids32), N, ptr(means), ptr(sums), ptr(sq), ptr(fg), st),
                          "gnms_bbox_stats_partials")
        return (sums if means is None else sq), fg

    def finish(self, deviation, partial, fg, count, out):
        with _lib.on_device(self.dev):
            check(self.lib.gnms_bbox_stats_finish(int(deviation), ptr(self.used), self.N, None if deviation else ptr(partial),
                                                  ptr(partial) if deviation else None, ptr(fg), ptr(count), ptr(out), stream_ptr(self.dev)),
                  "gnms_bbox_stats_finish")


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def image_partials(conf, imdb, use_trunc, means=None, batch_size=DEFAULT_BATCH, visit_order=None, device=None):
    """One pass's per-image partials, for tests and diagnosis: Partials(sums float32 [N, 13] (means None) or None, sq_sums float64
    [N, 13] (means given: 13 float64) or None, counts int32 [N], used bool [N]) as host arrays.  Rows of images without ground truths
    (used False) are not written by the device and come back as zeros."""
    _check_conf(conf, "image_partials")
    dev = _device(device)
    p = _Pass(conf, pack_records(conf, imdb), dev)
    m = None if means is None else torch.from_numpy(np.ascontiguousarray(np.asarray(means, np.float64).reshape(-1)[:STAT_COLS])).to(dev)
    part, fg = p.run(use_trunc, m, batch_size, visit_order)
    used = p.packed.counts > 0
    part, fg = part.cpu().numpy(), fg.cpu().numpy()
    part[~used] = 0
    fg[~used] = 0
    return Partials(part if means is None else None, part if means is not None else None, fg, used)


def compute_bbox_stats(conf, imdb, cache_folder="", *, batch_size=DEFAULT_BATCH, visit_order=None, device=None):
    """lib/rpn_util.py:547-736 on the GPU: sets conf.bbox_means and conf.bbox_stds (float64 [1, 13]).  batch_size: images per launch
    within a group of one feat_size (None or 0: the whole group); visit_order: the order the images are visited in (a permutation of
    range(len(imdb)); default imdb order).  Neither changes a bit of the result."""
    _check_conf(conf, "compute_bbox_stats")
    if (cache_folder is not None) and os.path.exists(os.path.join(cache_folder, "bbox_means.pkl")) \
            and os.path.exists(os.path.join(cache_folder, "bbox_stds.pkl")):
        conf["bbox_means"] = _pickle_read(os.path.join(cache_folder, "bbox_means.pkl"))
        conf["bbox_stds"] = _pickle_read(os.path.join(cache_folder, "bbox_stds.pkl"))
        return
    dev = _device(device)
    p = _Pass(conf, pack_records(conf, imdb), dev)
    result = torch.empty((2, STAT_COLS), dtype=torch.float64, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    logging.info("Computing bbox regression mean..")
    sums, fg = p.run(True, None, batch_size, visit_order)                              # :585-652
    p.finish(0, sums, fg, count, result[0])
    logging.info("Computing bbox regression stds..")
    sq, fg = p.run(False, result[0], batch_size, visit_order)                          # :659-721
    p.finish(1, sq, fg, count, result[1])
    host = result.cpu().numpy()                                                        # the one read
    means, stds = host[0:1].copy(), host[1:2].copy()
    if cache_folder is not None:
        _pickle_write(os.path.join(cache_folder, "bbox_means.pkl"), means)
        _pickle_write(os.path.join(cache_folder, "bbox_stds.pkl"), stds)
    conf["bbox_means"] = means
    conf["bbox_stds"] = stds
