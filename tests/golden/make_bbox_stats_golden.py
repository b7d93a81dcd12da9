"""Generate tests/golden/bbox_stats.npz by IMPORTING the reference's generate_anchors (lib/rpn_util.py:24-216) and compute_bbox_stats
(:547-736) and running them, with cache_folder=None, on a small synthetic imdb built here.  Runs only where the reference checkout is
(the first argument, read-only); it writes data only: the imdb as plain arrays, the conf values, the reference's anchors / bbox_means /
bbox_stds and, per image and pass, what compute_bbox_stats adds up -- the filtered ground truths, the foreground anchor indices and the
float32 column sums -- obtained by calling the reference's determine_ignores / locate_anchors / compute_targets the way
compute_bbox_stats does.

The reference's lib/rpn_util.py imports cv2, torchvision, PIL, lib.augmentations and the compiled lib.nms.gpu_nms at module top; none of
them is used here, so they are stubbed.  usage: python tests/golden/make_bbox_stats_golden.py REFERENCE_CHECKOUT"""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bbox_stats.npz")
COLUMNS = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13)


class _Stub(types.ModuleType):
    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return object


def load_reference():
    for name in ("cv2", "torchvision", "torchvision.transforms", "easydict", "shapely", "shapely.geometry", "visdom",
                 "lib.augmentations", "lib.nms", "lib.nms.gpu_nms"):
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules["lib.nms.gpu_nms"].gpu_nms = None
    sys.path.insert(0, REF)
    import lib.rpn_util as rpn_util   # noqa: E402
    return rpn_util


class Obj(dict):
    """what easydict gives the reference: keys as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def make_conf():
    return Obj(anchor_scales=[12.0, 20.0, 33.0, 56.0], anchor_ratios=[0.5, 1.0, 1.5], feat_stride=16, test_scale=96, has_3d=True,
               decomp_alpha=True, lbls=["Car", "Pedestrian"], ilbls=["Van", "DontCare"], min_gt_vis=0.65, min_gt_h=8.0, max_gt_h=10e10,
               fg_thresh=0.5, ign_thresh=0.5, bg_thresh_lo=0.0, bg_thresh_hi=0.5, best_thresh=0.35)


SIZES = ((375, 1242, 1.0), (370, 1300, 1.0), (375, 1242, 1.25))          # imH, imW, imobj.scale -> feat_size (6, 20), (6, 22), (8, 25)
DROPPED = (56.0, 0.5)                                                     # the candidate anchor no ground truth is made for


def make_gt(rng, conf, scale_factor, imH, imW, h_scaled, ratio, cls="Car", ign=False, vis=1.0, trunc=0.0):
    """a ground truth whose box, once scaled, is about h_scaled high and ratio * h_scaled wide, inside the image"""
    h = h_scaled * rng.uniform(0.93, 1.07) / scale_factor
    w = h_scaled * ratio * rng.uniform(0.93, 1.07) / scale_factor
    x = rng.uniform(0, max(imW - w - 1, 1))
    y = rng.uniform(0, max(imH - h - 1, 1))
    b3 = np.zeros(16)
    b3[0:2] = (x + w / 2 + rng.normal(0, 2), y + h / 2 + rng.normal(0, 2))                # projected centre
    b3[2] = rng.uniform(5, 60)                                                            # z
    b3[3:6] = rng.uniform(0.5, 4.5, 3)                                                    # w3d h3d l3d
    b3[6] = rng.uniform(-3.1, 3.1)                                                        # rotY
    b3[7:11] = rng.normal(0, 1, 4)
    b3[11] = rng.uniform(-3.1, 3.1)
    b3[12], b3[13] = np.sin(b3[11]), np.cos(b3[11])
    b3[14:16] = rng.normal(0, 1, 2)
    return Obj(cls=cls, ign=ign, visibility=vis, trunc=trunc, bbox_full=np.array([x, y, w, h]), bbox_3d=b3)


def make_imdb(rng, conf):
    shapes = [(s, r) for s in conf.anchor_scales for r in conf.anchor_ratios if (s, r) != DROPPED]
    todo = shapes * 2                                                     # every kept anchor is aimed at twice
    rng.shuffle(todo)
    imdb = []
    for k in range(10):
        imH, imW, scale = SIZES[k % 3]
        im = Obj(imH=imH, imW=imW, scale=scale, gts=[])
        sf = scale * conf.test_scale / imH
        mk = lambda hs, r, **kw: make_gt(rng, conf, sf, imH, imW, hs, r, **kw)            # noqa: E731
        if k == 3:
            pass                                                          # no gts: skipped (:587)
        elif k == 6:                                                      # all ignored or removed: no foreground, not skipped
            im.gts = [mk(33.0, 1.0, cls="Van"), mk(20.0, 1.5, cls="Tram"), mk(33.0, 0.5, vis=0.2), mk(20.0, 1.0, ign=True)]
        else:
            for _ in range(3):
                if todo:
                    hs, r = todo.pop()
                    im.gts.append(mk(hs, r, cls="Car" if rng.random() < 0.6 else "Pedestrian"))
            if k == 1:
                im.gts.insert(1, mk(33.0, 1.5, cls="Van"))                # a class of ilbls
                im.gts.insert(3, mk(5.0, 1.0))                            # too small after scaling
                im.gts.append(mk(20.0, 0.5, cls="Cyclist"))               # a class in neither list
            if k in (2, 7):
                im.gts.insert(2, mk(33.0, 1.0, trunc=0.6))                # trunc > max(1 - min_gt_vis, 0), otherwise valid
        imdb.append(im)
    assert not todo
    return imdb


def per_image(rpn_util, conf, imdb, use_trunc):
    """what one pass of compute_bbox_stats sees per image (:585-650 / :659-719)"""
    out = []
    for imobj in imdb:
        if len(imobj.gts) == 0:
            out.append(None)
            continue
        scale_factor = imobj.scale * conf.test_scale / imobj.imH
        feat_size = rpn_util.calc_output_size(np.array([imobj.imH, imobj.imW]) * scale_factor, conf.feat_stride)
        rois = rpn_util.locate_anchors(conf.anchors, feat_size, conf.feat_stride)
        igns, rmvs = rpn_util.determine_ignores(imobj.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, scale_factor,
                                                use_trunc=use_trunc)
        gts_all = rpn_util.bbXYWH2Coords(np.array([gt.bbox_full * scale_factor for gt in imobj.gts]))
        gts_val = gts_all[(rmvs == False) & (igns == False), :]                           # noqa: E712
        gts_ign = gts_all[(rmvs == False) & (igns == True), :]                            # noqa: E712
        box_lbls = np.array([gt.cls for gt in imobj.gts])
        box_lbls = box_lbls[(rmvs == False) & (igns == False)]                            # noqa: E712
        box_lbls = np.array([rpn_util.clsName2Ind(conf.lbls, cls) for cls in box_lbls])
        gts_3d = np.array([gt.bbox_3d for gt in imobj.gts])
        gts_3d = gts_3d[(rmvs == False) & (igns == False), :]                             # noqa: E712
        for gtind, gt in enumerate(gts_3d):
            gts_3d[gtind, 0:2] *= scale_factor
        transforms, _, _ = rpn_util.compute_targets(gts_val, gts_ign, box_lbls, rois, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo,
                                                    conf.bg_thresh_hi, conf.best_thresh, gts_3d=gts_3d, anchors=conf.anchors,
                                                    tracker=rois[:, 4])
        gt_inds = np.flatnonzero(transforms[:, 4] > 0)
        sums = np.zeros(13, np.float32)
        if len(gt_inds) > 0:
            sums[0:4] = np.sum(transforms[gt_inds, 0:4], axis=0)
            sums[4:] = np.sum(transforms[gt_inds, 5:14], axis=0)
            assert np.sum(transforms[gt_inds, 0:4], axis=0).dtype == np.float32
        out.append(dict(feat_size=feat_size, rois_dtype=rois.dtype, gts_val=gts_val, gts_ign=gts_ign, gts_3d=gts_3d, box_lbls=box_lbls,
                        fg=gt_inds, sums=sums, rows=transforms[gt_inds][:, COLUMNS]))
    return out


def main():
    if not REF:
        sys.exit(__doc__)
    rpn_util = load_reference()
    rng = np.random.default_rng(2027)
    conf = make_conf()
    imdb = make_imdb(rng, conf)
    N = len(imdb)
    z = {}
    # the imdb as plain arrays
    z["imdb/imH"] = np.array([im.imH for im in imdb], np.int64)
    z["imdb/imW"] = np.array([im.imW for im in imdb], np.int64)
    z["imdb/scale"] = np.array([im.scale for im in imdb], np.float64)
    z["imdb/n_gts"] = np.array([len(im.gts) for im in imdb], np.int64)
    flat = [gt for im in imdb for gt in im.gts]
    z["imdb/cls"] = np.array([gt.cls for gt in flat])
    z["imdb/ign"] = np.array([gt.ign for gt in flat], bool)
    z["imdb/visibility"] = np.array([gt.visibility for gt in flat], np.float64)
    z["imdb/trunc"] = np.array([gt.trunc for gt in flat], np.float64)
    z["imdb/bbox_full"] = np.array([gt.bbox_full for gt in flat], np.float64)
    z["imdb/bbox_3d"] = np.array([gt.bbox_3d for gt in flat], np.float64)
    for k, v in conf.items():
        z["conf/" + k] = np.array(v)

    # the reference, as scripts/train_rpn_3d.py:76-79 calls it
    rpn_util.generate_anchors(conf, imdb, None)
    assert conf.anchors.dtype == np.float64 and conf.anchors.shape == (11, 11), conf.anchors.shape
    kept = [(s, r) for s in conf.anchor_scales for r in conf.anchor_ratios if (s, r) != DROPPED]
    cand = np.array([rpn_util.anchor_center(s * r, s, conf.feat_stride) for s, r in kept], np.float32)
    assert np.array_equal(conf.anchors[:, 0:4], cand.astype(np.float64)), "another anchor than the intended one was dropped"
    rpn_util.compute_bbox_stats(conf, imdb, None)
    assert conf.bbox_means.dtype == np.float64 and conf.bbox_means.shape == (1, 13) and conf.bbox_stds.shape == (1, 13)
    z["anchors"], z["bbox_means"], z["bbox_stds"] = conf.anchors, conf.bbox_means, conf.bbox_stds

    # how many ground truths each kept anchor got (:119-138), restated from the reference's own pieces
    normalized = []
    for im in imdb:
        if len(im.gts) == 0:
            continue
        sf = im.scale * conf.test_scale / im.imH
        igns, rmvs = rpn_util.determine_ignores(im.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, sf)
        g = rpn_util.bbXYWH2Coords(np.array([gt.bbox_full * sf for gt in im.gts]))[(rmvs == False) & (igns == False), :]   # noqa: E712
        for row in g:
            normalized.append(rpn_util.anchor_center(row[2] - row[0] + 1, row[3] - row[1] + 1, conf.feat_stride))
    all12 = np.array([rpn_util.anchor_center(s * r, s, conf.feat_stride) for s in conf.anchor_scales for r in conf.anchor_ratios], np.float64)
    ols = rpn_util.iou(all12, np.array(normalized, np.float64))
    per_anchor = np.bincount(np.argmax(ols, axis=0)[np.amax(ols, axis=0) > 0.2], minlength=12)
    assert per_anchor.min() == 0 and np.sort(per_anchor)[1] >= 2, per_anchor
    z["gts_per_candidate_anchor"] = per_anchor

    differ = False
    for name, use_trunc in (("mean", True), ("dev", False)):
        imgs = per_image(rpn_util, conf, imdb, use_trunc)
        assert all(i is None or i["rois_dtype"] == np.float64 for i in imgs)               # locate_anchors(convert_tensor=False)
        z[name + "/feat_size"] = np.array([i["feat_size"] if i else (0, 0) for i in imgs], np.int64)
        z[name + "/fg_counts"] = np.array([len(i["fg"]) if i else 0 for i in imgs], np.int64)
        z[name + "/fg"] = np.concatenate([i["fg"] if i else np.zeros(0, np.int64) for i in imgs]).astype(np.int64)
        z[name + "/sums"] = np.stack([i["sums"] if i else np.zeros(13, np.float32) for i in imgs])
        z[name + "/rows"] = np.concatenate([i["rows"] if i else np.zeros((0, 13), np.float32) for i in imgs])
        for f, w in (("gts_val", 4), ("gts_ign", 4), ("gts_3d", 16)):
            z[name + "/" + f] = np.concatenate([i[f].reshape(-1, w) if i else np.zeros((0, w)) for i in imgs]).astype(np.float64)
            z[name + "/" + f + "_counts"] = np.array([len(i[f]) if i else 0 for i in imgs], np.int64)
        z[name + "/box_lbls"] = np.concatenate([i["box_lbls"] if i else np.zeros(0, np.int64) for i in imgs]).astype(np.int64)
    for k in range(N):
        differ |= z["mean/fg_counts"][k] != z["dev/fg_counts"][k]
    assert differ, "the two passes select the same foreground: the trunc ground truths do not bite"
    assert len(set(map(tuple, z["mean/feat_size"][z["imdb/n_gts"] > 0]))) >= 2
    assert z["dev/fg_counts"].max() < 2 ** 13
    # the reference's own sum is what compute_bbox_stats divides: check the stored sums against its means
    n = z["mean/fg_counts"].sum()
    s64 = z["mean/sums"].astype(np.float64)
    assert np.all(np.abs(s64.sum(0) / n - conf.bbox_means[0]) <= 1e-12 * np.abs(s64).sum(0) / n), (s64.sum(0) / n, conf.bbox_means[0])

    # an imdb without any foreground: the reference divides 0 by 1e-10
    conf2 = make_conf()
    conf2.anchors = conf.anchors
    rpn_util.compute_bbox_stats(conf2, [imdb[6], imdb[3]], None)
    z["nofg/bbox_means"], z["nofg/bbox_stds"] = conf2.bbox_means, conf2.bbox_stds
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes); A=%d, fg per image mean pass %s, dev pass %s" % (
        OUT, len(z), os.path.getsize(OUT), conf.anchors.shape[0], z["mean/fg_counts"].tolist(), z["dev/fg_counts"].tolist()))


if __name__ == "__main__":
    main()
