"""The KITTI evaluation (groomed_nms_amd.kitti_eval, csrc/kitti_eval.hip) without a GPU: the C ABI and its argument checks, the host
parsers and writers, and the yardstick the GPU tests compare against -- a line-for-line Python restatement of the devkit
(data/kitti_split1/devkit/cpp/evaluate_object.cpp: cleanData, computeStatistics, getThresholds, eval_class, eval and the three
overlap functions), loops and conditions in the devkit's order.  Its footprint intersection is test_iou3d_exact_host's checker (convex
hull of the mutual vertices and edge crossings), not the kernel's clip.  The restatement is pinned by hand-worked cases below.

The scene generators of the GPU tests live here as well, so that the margin condition on their seeds (every overlap the restatement
computes lies at least 1e-9 away from every min_overlap in use) is checked on the CPU."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from groomed_nms_amd import kitti_eval as K          # (the module under test: without it nothing here has a subject)
from test_iou3d_exact_host import _area, intersection_area

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gnms_kitti_eval_plan", "gnms_kitti_eval_recall", "gnms_kitti_eval_precision")

# ---------------------------------------------------------------------------------------------------------------------------
# the restatement (evaluate_object.cpp line numbers)
# ---------------------------------------------------------------------------------------------------------------------------
MIN_HEIGHT = [40, 25, 25]                 # :49
MAX_OCCLUSION = [0, 1, 2]                 # :50
MAX_TRUNCATION = [0.15, 0.3, 0.5]         # :51
CLASS_NAMES = ["car", "pedestrian", "cyclist"]
N_SAMPLE_PTS = 41.0
IMAGE, GROUND, BOX3D = 0, 1, 2
MARGIN = 1e-9


class MarginError(Exception):
    """an overlap within MARGIN of a min_overlap: the two clip algorithms could legitimately decide differently"""


def strcasecmp(a, b):
    return 0 if a.lower() == b.lower() else 1


def det(type, x1, y1, x2, y2, score, alpha=0.0, h=1.5, w=1.6, l=3.9, t=(0.0, 1.5, 20.0), ry=0.0):
    return SimpleNamespace(type=type, x1=float(x1), y1=float(y1), x2=float(x2), y2=float(y2), alpha=float(alpha), thresh=float(score), h=float(h),
                           w=float(w), l=float(l), t1=float(t[0]), t2=float(t[1]), t3=float(t[2]), ry=float(ry))


def gt(type, x1, y1, x2, y2, truncation=0.0, occlusion=0, alpha=0.0, h=1.5, w=1.6, l=3.9, t=(0.0, 1.5, 20.0), ry=0.0):
    return SimpleNamespace(type=type, x1=float(x1), y1=float(y1), x2=float(x2), y2=float(y2), alpha=float(alpha), truncation=float(truncation),
                           occlusion=int(occlusion), h=float(h), w=float(w), l=float(l), t1=float(t[0]), t2=float(t[1]), t3=float(t[2]), ry=float(ry))


def dontcare(x1, y1, x2, y2):
    return gt("DontCare", x1, y1, x2, y2, truncation=-1, occlusion=-1, alpha=-10, h=-1, w=-1, l=-1, t=(-1000, -1000, -1000), ry=-10)


def imageBoxOverlap(a, b, criterion=-1):                                        # :247-281
    x1 = max(a.x1, b.x1)
    y1 = max(a.y1, b.y1)
    x2 = min(a.x2, b.x2)
    y2 = min(a.y2, b.y2)
    w = x2 - x1
    h = y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    a_area = (a.x2 - a.x1) * (a.y2 - a.y1)
    b_area = (b.x2 - b.x1) * (b.y2 - b.y1)
    if criterion == -1:
        return inter / (a_area + b_area - inter)
    return inter / a_area


def toPolygon(g):                                                               # :289-311
    c, s = math.cos(g.ry), math.sin(g.ry)
    xs = [g.l / 2, g.l / 2, -g.l / 2, -g.l / 2]
    zs = [g.w / 2, -g.w / 2, -g.w / 2, g.w / 2]
    return [((c * xs[i] + s * zs[i]) + g.t1, (-s * xs[i] + c * zs[i]) + g.t3) for i in range(4)]


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _inter_area(d, g):
    return intersection_area(toPolygon(g), toPolygon(d))


def groundBoxOverlap(d, g, criterion=-1):                                       # :314-334 (union area = the two areas minus the intersection)
    inter_area = _inter_area(d, g)
    d_area, g_area = abs(_area(toPolygon(d))), abs(_area(toPolygon(g)))
    if criterion == -1:
        return _div(inter_area, (d_area + g_area) - inter_area)
    return _div(inter_area, d_area)


def box3DOverlap(d, g, criterion=-1):                                           # :337-364
    ymax = min(d.t2, g.t2)
    ymin = max(d.t2 - d.h, g.t2 - g.h)
    inter_area = _inter_area(d, g)
    inter_vol = inter_area * max(0.0, ymax - ymin)
    det_vol = d.h * d.l * d.w
    gt_vol = g.h * g.l * g.w
    if criterion == -1:
        return _div(inter_vol, det_vol + gt_vol - inter_vol)
    return _div(inter_vol, det_vol)


BOXOVERLAP = (imageBoxOverlap, groundBoxOverlap, box3DOverlap)


def getThresholds(v, n_groundtruth):                                            # :366-399
    t = []
    v.sort(reverse=True)
    current_recall = 0.0
    for i in range(len(v)):
        l_recall = float(i + 1) / n_groundtruth
        if i < len(v) - 1:
            r_recall = float(i + 2) / n_groundtruth
        else:
            r_recall = l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current_recall += 1.0 / (N_SAMPLE_PTS - 1.0)
    return t


def cleanData(current_class, gts, dets, difficulty, max_depth):                 # :401-474
    ignored_gt, dc, ignored_det, n_gt = [], [], [], 0
    for g in gts:
        height = g.y2 - g.y1
        if not strcasecmp(g.type, CLASS_NAMES[current_class]):
            valid_class = 1
        elif not strcasecmp(CLASS_NAMES[current_class], "Pedestrian") and not strcasecmp("Person_sitting", g.type):
            valid_class = 0
        elif not strcasecmp(CLASS_NAMES[current_class], "Car") and not strcasecmp("Van", g.type):
            valid_class = 0
        else:
            valid_class = -1
        ignore = False
        if (g.occlusion > MAX_OCCLUSION[difficulty] or g.truncation > MAX_TRUNCATION[difficulty] or height <= MIN_HEIGHT[difficulty]
                or (max_depth is not None and g.t3 > max_depth)):               # the _<D>m_ variants: || gt[i].t3 > D
            ignore = True
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            n_gt += 1
        elif valid_class == 0 or (ignore and valid_class == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
    for i, g in enumerate(gts):
        if not strcasecmp("DontCare", g.type):
            dc.append(i)                                                        # (the row's index: dc[k] is gts[dc[k]])
    for d in dets:
        if not strcasecmp(d.type, CLASS_NAMES[current_class]):
            valid_class = 1
        else:
            valid_class = -1
        height = int(math.fabs(d.y1 - d.y2))                                    # int32_t height = fabs(...): truncated
        if height < MIN_HEIGHT[difficulty]:
            ignored_det.append(1)
        elif valid_class == 1:
            ignored_det.append(0)
        else:
            ignored_det.append(-1)
    return ignored_gt, dc, ignored_det, n_gt


def computeStatistics(gts, dets, dc, ignored_gt, ignored_det, compute_fp, boxoverlap, min_overlap, compute_aos=False, thresh=0.0):   # :476-634
    stat = SimpleNamespace(v=[], similarity=0.0, tp=0, fp=0, fn=0)
    NO_DETECTION = -10000000
    delta = []
    assigned_detection = [False] * len(dets)
    ignored_threshold = [False] * len(dets)
    if compute_fp:
        for i in range(len(dets)):
            if dets[i].thresh < thresh:
                ignored_threshold[i] = True
    for i in range(len(gts)):
        if ignored_gt[i] == -1:
            continue
        det_idx = -1
        valid_detection = NO_DETECTION
        max_overlap = 0.0
        assigned_ignored_det = False
        for j in range(len(dets)):
            if ignored_det[j] == -1:
                continue
            if assigned_detection[j]:
                continue
            if ignored_threshold[j]:
                continue
            overlap = boxoverlap(j, i, -1)
            if not compute_fp and overlap > min_overlap and dets[j].thresh > valid_detection:
                det_idx = j
                valid_detection = dets[j].thresh
            elif compute_fp and overlap > min_overlap and (overlap > max_overlap or assigned_ignored_det) and ignored_det[j] == 0:
                max_overlap = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif compute_fp and overlap > min_overlap and valid_detection == NO_DETECTION and ignored_det[j] == 1:
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True
        if valid_detection == NO_DETECTION and ignored_gt[i] == 0:
            stat.fn += 1
        elif valid_detection != NO_DETECTION and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned_detection[det_idx] = True
        elif valid_detection != NO_DETECTION:
            stat.tp += 1
            stat.v.append(dets[det_idx].thresh)
            if compute_aos:
                delta.append(gts[i].alpha - dets[det_idx].alpha)
            assigned_detection[det_idx] = True
    if compute_fp:
        for i in range(len(dets)):
            if not (assigned_detection[i] or ignored_det[i] == -1 or ignored_det[i] == 1 or ignored_threshold[i]):
                stat.fp += 1
        nstuff = 0
        for i in range(len(dc)):
            for j in range(len(dets)):
                if assigned_detection[j]:
                    continue
                if ignored_det[j] == -1 or ignored_det[j] == 1:
                    continue
                if ignored_threshold[j]:
                    continue
                overlap = boxoverlap(j, dc[i], 0)
                if overlap > min_overlap:
                    assigned_detection[j] = True
                    nstuff += 1
        stat.fp -= nstuff
        if compute_aos:
            tmp = [0.0] * stat.fp
            for d in delta:
                tmp.append((1.0 + math.cos(d)) / 2.0)
            assert len(tmp) == stat.fp + stat.tp and len(delta) == stat.tp
            if stat.tp > 0 or stat.fp > 0:
                acc = 0.0
                for x in tmp:
                    acc = acc + x
                stat.similarity = acc
            else:
                stat.similarity = -1
    return stat


class Overlaps:
    """boxoverlap(det[j], gt[i], criterion) of one image and metric, computed once per argument triple (the devkit recomputes it at
    every threshold) and recorded for the margin check and the comparison with the device's matrices"""

    def __init__(self, gts, dets, metric):
        self.gts, self.dets, self.fn, self.memo = gts, dets, BOXOVERLAP[metric], {}

    def __call__(self, j, i, criterion):
        key = (j, i, criterion)
        if key not in self.memo:
            self.memo[key] = self.fn(self.dets[j], self.gts[i], criterion)
        return self.memo[key]


def eval_class(current_class, scene, compute_aos, metric, difficulty, min_overlap, max_depth, overlaps):      # :640-724
    n_gt = 0
    v = []
    cleaned = []
    for (gts, dets), ov in zip(scene, overlaps):
        i_gt, dc, i_det, n = cleanData(current_class, gts, dets, difficulty, max_depth)
        n_gt += n
        cleaned.append((i_gt, dc, i_det))
        pr_tmp = computeStatistics(gts, dets, dc, i_gt, i_det, False, ov, min_overlap)
        v.extend(pr_tmp.v)
    thresholds = getThresholds(v, n_gt)
    pr = [SimpleNamespace(similarity=0.0, tp=0, fp=0, fn=0) for _ in thresholds]
    for (gts, dets), ov, (i_gt, dc, i_det) in zip(scene, overlaps, cleaned):
        for t in range(len(thresholds)):
            tmp = computeStatistics(gts, dets, dc, i_gt, i_det, True, ov, min_overlap, compute_aos, thresholds[t])
            pr[t].tp += tmp.tp
            pr[t].fp += tmp.fp
            pr[t].fn += tmp.fn
            if tmp.similarity != -1:
                pr[t].similarity += tmp.similarity
    precision = [0.0] * int(N_SAMPLE_PTS)
    aos = [0.0] * int(N_SAMPLE_PTS) if compute_aos else None
    for i in range(len(thresholds)):
        precision[i] = _div(pr[i].tp, float(pr[i].tp + pr[i].fp))
        if compute_aos:
            aos[i] = _div(pr[i].similarity, float(pr[i].tp + pr[i].fp))
    for i in range(len(thresholds)):
        precision[i] = max(precision[i:])
        if compute_aos:
            aos[i] = max(aos[i:])
    return SimpleNamespace(n_gt=n_gt, thresholds=thresholds, tp=[p.tp for p in pr], fp=[p.fp for p in pr], fn=[p.fn for p in pr],
                           precision=precision, aos=aos)


def load_switches(scene):                                                       # loadDetections (:150-196) over all images
    compute_aos = True
    eval_image, eval_ground, eval_3d = [False] * 3, [False] * 3, [False] * 3
    for _, dets in scene:
        for d in dets:
            if d.alpha == -10:
                compute_aos = False
            for c in range(3):
                if not strcasecmp(d.type, CLASS_NAMES[c]):
                    if not eval_image[c] and d.x1 >= 0:
                        eval_image[c] = True
                    if not eval_ground[c] and d.t1 != -1000 and d.t3 != -1000 and d.w > 0 and d.l > 0:
                        eval_ground[c] = True
                    if not eval_3d[c] and d.t1 != -1000 and d.t2 != -1000 and d.t3 != -1000 and d.h > 0 and d.w > 0 and d.l > 0:
                        eval_3d[c] = True
                    break
    return compute_aos, eval_image, eval_ground, eval_3d


def ref_eval(scene, variants, margin=MARGIN):
    """eval() (:791-926) for each (min_overlap [3][3], max_depth) variant.  Returns (switches, overlaps, [curves per variant]): curves
    maps (class, metric, difficulty) to eval_class's result, only for the curves that are on; overlaps[metric][image] is the memo.
    Raises MarginError if an overlap it used lies within `margin` of a min_overlap of the variants."""
    compute_aos, eval_image, eval_ground, eval_3d = load_switches(scene)
    overlaps = [[Overlaps(gts, dets, metric) for gts, dets in scene] for metric in range(3)]
    out = []
    for min_overlap, max_depth in variants:
        curves = {}
        for metric, on in ((IMAGE, eval_image), (GROUND, eval_ground), (BOX3D, eval_3d)):
            for c in range(3):
                if on[c]:
                    for difficulty in range(3):
                        curves[(c, metric, difficulty)] = eval_class(c, scene, compute_aos and metric == IMAGE, metric, difficulty,
                                                                     min_overlap[metric][c], max_depth, overlaps[metric])
        out.append(curves)
    mins = sorted({m for mo, _ in variants for row in mo for m in row})
    for per_image in overlaps:
        for ov in per_image:
            for o in ov.memo.values():
                if any(abs(o - m) < margin for m in mins):
                    raise MarginError(o)
    return SimpleNamespace(compute_aos=compute_aos, eval_image=eval_image, eval_ground=eval_ground, eval_3d=eval_3d), overlaps, out


# ---------------------------------------------------------------------------------------------------------------------------
# scenes -> the packed arrays / the folders
# ---------------------------------------------------------------------------------------------------------------------------
TYPE_IDS = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}


def pack(scene):
    """(det [n, 14], det_offsets, gt [m, 15], gt_offsets) in the documented row layout"""
    drows, grows, doff, goff = [], [], [0], [0]
    for gts, dets in scene:
        for d in dets:
            cid = TYPE_IDS.get(d.type.lower(), -1)
            drows.append([cid if cid in (0, 1, 2) else -1, d.alpha, d.x1, d.y1, d.x2, d.y2, d.h, d.w, d.l, d.t1, d.t2, d.t3, d.ry, d.thresh])
        for g in gts:
            grows.append([TYPE_IDS.get(g.type.lower(), 6), g.truncation, g.occlusion, g.alpha, g.x1, g.y1, g.x2, g.y2, g.h, g.w, g.l, g.t1, g.t2,
                          g.t3, g.ry])
        doff.append(len(drows))
        goff.append(len(grows))
    return (np.array(drows, np.float64).reshape(-1, 14), np.array(doff, np.int32), np.array(grows, np.float64).reshape(-1, 15),
            np.array(goff, np.int32))


def write_folders(scene, root):
    """<root>/results/data/%06d.txt and <root>/label_2/%06d.txt with 6 decimals (what the project's writer emits); returns the two paths"""
    res, lab = os.path.join(root, "results", "data"), os.path.join(root, "label_2")
    os.makedirs(res)
    os.makedirs(lab)
    for k, (gts, dets) in enumerate(scene):
        with open(os.path.join(res, "%06d.txt" % k), "w") as f:
            for d in dets:
                f.write(("%s -1 -1" + " %.6f" * 13 + "\n") % (d.type, d.alpha, d.x1, d.y1, d.x2, d.y2, d.h, d.w, d.l, d.t1, d.t2, d.t3, d.ry, d.thresh))
        with open(os.path.join(lab, "%06d.txt" % k), "w") as f:
            for g in gts:
                f.write(("%s %.6f %d" + " %.6f" * 12 + "\n") % (g.type, g.truncation, g.occlusion, g.alpha, g.x1, g.y1, g.x2, g.y2, g.h, g.w, g.l,
                                                                g.t1, g.t2, g.t3, g.ry))
    return os.path.join(root, "results"), lab


def rounded6(scene):
    """the scene as it reads back from write_folders' files"""
    def r(x):
        return float("%.6f" % x)
    out = []
    for gts, dets in scene:
        out.append(([gt(g.type, r(g.x1), r(g.y1), r(g.x2), r(g.y2), r(g.truncation), g.occlusion, r(g.alpha), r(g.h), r(g.w), r(g.l),
                        (r(g.t1), r(g.t2), r(g.t3)), r(g.ry)) for g in gts],
                    [det(d.type, r(d.x1), r(d.y1), r(d.x2), r(d.y2), r(d.thresh), r(d.alpha), r(d.h), r(d.w), r(d.l), (r(d.t1), r(d.t2), r(d.t3)),
                         r(d.ry)) for d in dets]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# scene generators (shared with the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
def _project(rng, x, z, h):
    """a plausible image box for an object at (x, z): 720 px focal length, bottom at 250 px"""
    u = 620.0 + 720.0 * x / z
    hp = 720.0 * h / z
    wp = hp * rng.uniform(0.8, 2.0)
    return u - wp / 2, 250.0 - hp, u + wp / 2, 250.0


def random_image(rng, n_gt, n_det, classes=("Car",), neighbours=True, n_dc=1, tie_scores=False, depth=(6.0, 70.0), easy=False):
    """n_gt objects, detections that jitter them (two per object every third object -> competing candidates), clutter, DontCare boxes"""
    gts, dets = [], []
    for k in range(n_gt):
        cls = classes[int(rng.integers(len(classes)))]
        if neighbours and rng.uniform() < 0.15:
            cls = {"Car": "Van", "Pedestrian": "Person_sitting"}.get(cls, "Tram")
        z = rng.uniform(*depth)
        x = rng.uniform(-0.45, 0.45) * z
        h, w, l = (rng.uniform(1.4, 1.9), rng.uniform(1.5, 1.9), rng.uniform(3.2, 4.6)) if cls in ("Car", "Van", "Tram") else \
            (rng.uniform(1.5, 1.9), rng.uniform(0.5, 0.8), rng.uniform(0.6, 1.8))
        x1, y1, x2, y2 = _project(rng, x, z, h)
        trunc, occ = float(rng.choice([0.0, 0.1, 0.15, 0.2, 0.3, 0.31, 0.5, 0.6])), int(rng.integers(0, 4))
        gts.append(gt(cls if rng.uniform() < 0.8 else cls.upper(), x1, y1, x2, y2, truncation=0.0 if easy else trunc, occlusion=0 if easy else occ, alpha=rng.uniform(-math.pi, math.pi), h=h, w=w, l=l, t=(x, 1.6, z),
                      ry=rng.uniform(-math.pi, math.pi)))
    for k in range(n_det):
        if gts and k < 2 * len(gts):
            g = gts[k % len(gts)]
            s = rng.uniform(0.0, 0.12) if k < len(gts) else rng.uniform(0.05, 0.3)
            cls = g.type.capitalize() if g.type.lower() in CLASS_NAMES else classes[0]
            bw, bh = g.x2 - g.x1, g.y2 - g.y1
            d = det(cls, g.x1 + s * bw * rng.uniform(-1, 1), g.y1 + s * bh * rng.uniform(-1, 1), g.x2 + s * bw * rng.uniform(-1, 1),
                    g.y2 + s * bh * rng.uniform(-1, 1), 0.0, alpha=g.alpha + rng.uniform(-0.5, 0.5), h=g.h * (1 + s * rng.uniform(-1, 1)),
                    w=g.w * (1 + s * rng.uniform(-1, 1)), l=g.l * (1 + s * rng.uniform(-1, 1)),
                    t=(g.t1 + 2 * s * rng.uniform(-1, 1), g.t2 + s * rng.uniform(-1, 1), g.t3 + 4 * s * rng.uniform(-1, 1)),
                    ry=g.ry + s * rng.uniform(-2, 2))
        else:
            z = rng.uniform(*depth)
            x = rng.uniform(-0.45, 0.45) * z
            x1, y1, x2, y2 = _project(rng, x, z, 1.6)
            d = det(classes[int(rng.integers(len(classes)))], x1, y1, x2, y2, 0.0, alpha=rng.uniform(-3, 3), t=(x, 1.6, z), ry=rng.uniform(-3, 3))
        d.thresh = float(rng.integers(1, 20)) / 20.0 if tie_scores else float(rng.uniform(0.01, 1.0))
        dets.append(d)
    for _ in range(n_dc):
        x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 200)
        gts.insert(int(rng.integers(0, len(gts) + 1)), dontcare(x1, y1, x1 + rng.uniform(50, 400), y1 + rng.uniform(30, 120)))
    return gts, dets


def with_margin(make, variants, first_seed):
    """the first seed >= first_seed whose scene satisfies the margin condition: (seed, scene, reference)"""
    for seed in range(first_seed, first_seed + 50):
        scene = make(np.random.default_rng(seed))
        try:
            return seed, scene, ref_eval(scene, variants)
        except MarginError:
            continue
    raise AssertionError("no seed with margin")


MAIN = (((0.7, 0.5, 0.5),) * 3, None)
SIDE = (((0.5, 0.3, 0.3),) * 3, None)


def grid(d, v):
    return (((v, v, v),) * 3, float(d))


def scene_mixed(rng):
    """all three classes with neighbours, rotated footprints, DontCare, a few images; plus an image without detections, one without
    ground truth, one with DontCare only"""
    scene = [random_image(rng, int(rng.integers(3, 9)), int(rng.integers(4, 14)), classes=("Car", "Pedestrian", "Cyclist"), n_dc=int(rng.integers(0, 3)))
             for _ in range(14)]
    scene.append((random_image(rng, 4, 0, classes=("Car", "Pedestrian"))[0], []))
    scene.append(([], random_image(rng, 0, 5, classes=("Car", "Cyclist"), n_dc=0)[1]))
    scene.append(([dontcare(100, 100, 400, 220), dontcare(500, 120, 900, 240)], random_image(rng, 0, 4, n_dc=0)[1]))
    return scene


def scene_words(rng):
    """70 and 130 detections of one class against 12 ground truths (one and two word boundaries of assigned_detection), tied scores"""
    return [random_image(rng, 12, 70, tie_scores=True, n_dc=2, depth=(8.0, 30.0)), random_image(rng, 12, 130, tie_scores=True, n_dc=2, depth=(8.0, 30.0)),
            ([gt("Cyclist", 100, 100, 160, 200)], [])]                          # a class that is never detected: its curves are absent


def scene_many(rng):
    """40 images, about 300 true positives of one class: getThresholds' skip branch, exactly 41 thresholds"""
    return [random_image(rng, 10, 12, neighbours=False, n_dc=1, depth=(6.0, 25.0), easy=True) for _ in range(40)]


def scene_rules(rng):
    """the ignore rules, hand-built (rng only draws the scores)"""
    def sc():
        return float(rng.uniform(0.05, 1.0))

    def at(k):                                                                  # distinct places on the ground, 6 m apart
        return (-24.0 + 6.0 * (k % 9), 1.5, 12.0 + 7.0 * (k // 9))
    scene = []
    # 0: box heights around both MIN_HEIGHTs: the ground truth compares the double with <=, the detection the truncated int with <
    gts, dets = [], []
    for k, hgt in enumerate((24.0, 25.0, 25.5, 39.9, 40.0, 40.5, 60.0)):
        gts.append(gt("Car", 150 * k, 100, 150 * k + 100, 100 + hgt, t=at(k)))
        dets.append(det("Car", 150 * k, 100, 150 * k + 100, 100 + hgt, sc(), t=at(k), alpha=0.3 * k))
    scene.append((gts, dets))
    # 1: assigned_ignored_det in the ground / 3D metric (the 3D boxes overlap, the image boxes decide who is ignored):
    #    G0: ignored-height candidate first, then a valid one (hand-over), then another ignored one (not taken);
    #    G1: valid first, ignored later; G2: an ignored-height candidate only (assigned: no tp, no fn)
    gts = [gt("Car", 100 + 250 * k, 100, 300 + 250 * k, 300, t=at(k)) for k in range(3)]
    small = dict(x1=900, y1=10, x2=1000, y2=30)
    dets = [det("Car", score=sc(), t=at(0), **small), det("Car", 110, 105, 310, 295, sc(), t=(at(0)[0] + 0.2, 1.5, at(0)[2])),
            det("Car", score=sc(), t=(at(0)[0] + 0.1, 1.5, at(0)[2]), **small),
            det("Car", 350, 100, 550, 300, sc(), t=(at(1)[0] + 0.3, 1.5, at(1)[2] + 0.1)), det("Car", score=sc(), t=at(1), **small),
            det("Car", score=sc(), t=at(2), **small)]
    scene.append((gts, dets))
    # 2: occlusion 0..3 x truncation around 0.15 / 0.3 / 0.5; every second one detected; Van neighbours absorbing detections
    gts, dets = [], []
    for k, (occ, trunc) in enumerate((o, t) for o in range(4) for t in (0.1, 0.15, 0.16, 0.3, 0.31, 0.5, 0.51)):
        box = (40 * (k % 14) * 2, 100 + 100 * (k // 14), 40 * (k % 14) * 2 + 60, 150 + 100 * (k // 14))
        gts.append(gt("Van" if k % 9 == 4 else "Car", *box, truncation=trunc, occlusion=occ, t=at(k), ry=0.1 * k))
        if k % 2 == 0:
            dets.append(det("Car", box[0] + 2, box[1], box[2] + 2, box[3], sc(), t=(at(k)[0] + 0.1, 1.5, at(k)[2]), ry=0.1 * k + 0.05, alpha=0.1 * k))
    scene.append((gts, dets))
    # 3: stuff areas: D1 = [0, 100], D2 = [55, 155] in x.  f1 inside D1; f2 45 / 80 in D1 (between the main and the side threshold) and
    #    inside D2; f3 inside both (nstuff counts it once); f4 22 / 80 in D2 only (stays a false positive); one true positive
    gts = [dontcare(0, 0, 100, 100), gt("Car", 400, 100, 500, 200, t=at(3)), dontcare(55, 0, 155, 100)]
    dets = [det("Car", 10, 10, 90, 90, sc(), t=at(10)), det("Car", 55, 10, 135, 90, sc(), t=at(11)), det("Car", 57, 10, 97, 90, sc(), t=at(12)),
            det("Car", 133, 10, 213, 90, sc(), t=at(13)), det("Car", 400, 100, 500, 200, sc(), t=at(3))]
    scene.append((gts, dets))
    # 4: Pedestrian / Person_sitting / Cyclist rows with their own thresholds, rotated
    gts = [gt("Pedestrian", 100, 100, 140, 200, h=1.8, w=0.6, l=0.8, t=at(0), ry=0.7), gt("Person_sitting", 200, 100, 260, 180, h=1.2, w=0.6, l=0.8, t=at(1)),
           gt("Cyclist", 300, 100, 360, 200, h=1.7, w=0.6, l=1.8, t=at(2), ry=-1.1), gt("Pedestrian", 500, 100, 540, 200, h=1.8, w=0.6, l=0.8, t=at(4), ry=2.0)]
    dets = [det("Pedestrian", 102, 104, 141, 199, sc(), h=1.75, w=0.6, l=0.8, t=(at(0)[0] + 0.05, 1.5, at(0)[2]), ry=0.8, alpha=1.0),
            det("Pedestrian", 200, 100, 260, 180, sc(), h=1.2, w=0.6, l=0.8, t=at(1)),
            det("Cyclist", 305, 100, 365, 200, sc(), h=1.7, w=0.6, l=1.8, t=(at(2)[0], 1.5, at(2)[2] + 0.1), ry=-1.0, alpha=-2.0),
            det("Pedestrian", 515, 100, 555, 200, sc(), h=1.8, w=0.6, l=0.8, t=(at(4)[0] + 0.2, 1.4, at(4)[2] + 0.1), ry=2.3),
            det("Cyclist", 700, 100, 760, 200, sc(), h=1.7, w=0.6, l=1.8, t=at(7))]
    scene.append((gts, dets))
    return scene


def scene_no3d(rng):
    """eval_ground / eval_3d switching: Pedestrian detections carry t = -1000 (ground and 3D off), Cyclist detections h = 0 (3D off);
    Car is complete"""
    scene = [random_image(rng, 5, 8, classes=("Car", "Pedestrian", "Cyclist"), neighbours=False, depth=(6.0, 30.0), easy=True) for _ in range(3)]
    for _, dets in scene:
        for d in dets:
            if d.type == "Pedestrian":
                d.t1 = d.t2 = d.t3 = -1000.0
            elif d.type == "Cyclist":
                d.h = 0.0
    return scene


def limits_case():
    """one image at the documented limits' lower bounds (512 detections, 64 ground truths) and the restatement of its moderate Car
    image curve under SIDE's 0.5; the margin condition holds for the overlaps that curve reads"""
    for seed in range(1, 50):
        gts, dets = random_image(np.random.default_rng(seed), 64, 512, n_dc=0, depth=(6.0, 25.0), easy=True, neighbours=False)
        ov = [Overlaps(gts, dets, IMAGE)]
        r = eval_class(0, [(gts, dets)], True, IMAGE, 1, 0.5, None, ov)
        if all(abs(o - m) >= MARGIN for o in ov[0].memo.values() for m in (0.5, 0.3)):
            return [(gts, dets)], r
    raise AssertionError("no seed with margin")


def test_limits_case_has_margin_at_its_first_seed():
    scene, r = limits_case()
    assert len(scene[0][1]) == 512 and len(scene[0][0]) == 64 and r.n_gt == 64 and len(r.thresholds) > 20
    assert max(t + f for t, f in zip(r.tp, r.fp)) <= 2000


# ---------------------------------------------------------------------------------------------------------------------------
# hand-worked pins
# ---------------------------------------------------------------------------------------------------------------------------
def test_pin_a_one_car_one_detection():
    """One easy Car (100 px high, occlusion 0, truncation 0) and one identical detection, score 0.9.  Every overlap is 1 > 0.7.
    Recall pass: tp scores [0.9], n_gt = 1.  getThresholds: i = 0 is the last score, l = r = 1, pushed: thresholds [0.9].  Precision
    pass at 0.9: tp = 1, fp = fn = 0, precision[0] = 1, the other 40 entries stay 0.  R40 (indices 1..40) = 0, R11 (0, 4, .., 40) = 1/11.
    alpha equal on both sides: similarity (1 + cos 0) / 2 = 1, aos[0] = 1."""
    scene = [([gt("Car", 100, 100, 200, 200)], [det("Car", 100, 100, 200, 200, 0.9)])]
    sw, _, (curves,) = ref_eval(scene, [MAIN])
    assert sw.compute_aos and sw.eval_image == [True, False, False] and sw.eval_ground == [True, False, False] and sw.eval_3d == [True, False, False]
    assert sorted(curves) == [(0, m, d) for m in range(3) for d in range(3)]
    for (c, m, d), r in curves.items():
        assert r.n_gt == 1 and r.thresholds == [0.9] and r.tp == [1] and r.fp == [0] and r.fn == [0]
        assert r.precision == [1.0] + [0.0] * 40
        assert (r.aos == [1.0] + [0.0] * 40) if m == IMAGE else r.aos is None
        assert np.mean(r.precision[1:41]) == 0.0 and np.mean(r.precision[0:41:4]) == 1.0 / 11.0


def pin_b_scene():
    far = dict(t=(30.0, 1.5, 60.0))
    img0_gt = [gt("Car", 100, 100, 200, 200, t=(0, 1.5, 20)), dontcare(400, 100, 500, 200)]
    img0_det = [det("Car", 100, 100, 200, 200, 0.9, t=(0, 1.5, 20)),            # d0: the Car itself
                det("Car", 410, 110, 490, 190, 0.8, t=(-30, 1.5, 60)),          # d1: inside the DontCare box, 3D box away from everything
                det("Car", 600, 100, 700, 200, 0.85, **far)]                    # d5: a plain false positive
    img1_gt = [gt("Van", 100, 100, 200, 200, t=(-5, 1.5, 30)), gt("Car", 300, 100, 400, 200, t=(5, 1.5, 30))]
    img1_det = [det("Car", 100, 100, 200, 200, 0.7, t=(-5, 1.5, 30)),           # d2: on the Van
                det("Car", 300, 100, 400, 124, 0.95, t=(40, 1.5, 60)),          # d3: 24 px high
                det("Car", 300, 100, 400, 200, 0.6, alpha=math.pi / 2, t=(5, 1.5, 30))]   # d4: the second Car
    return [(img0_gt, img0_det), (img1_gt, img1_det)]


def test_pin_b_dontcare_van_and_small_detection():
    """Two images, class Car, min_overlap 0.7, any difficulty (both Cars are easy; every detection but d3 is 80 or 100 px high).
    n_gt = 2 (the Van has ignored_gt = 1, DontCare -1).  Recall pass: the Car of image 0 takes d0 (0.9), the Van takes d2 (assigned,
    no tp), the Car of image 1 takes d4 (0.6; d3's IoU with it is 24/100).  Scores [0.9, 0.6].
    getThresholds, n_gt = 2: i = 0: l = 0.5, r = 1, current 0: (1 - 0) < (0 - 0.5) is false -> push 0.9, current = 0.025;
    i = 1 is the last -> push 0.6.
    Image metric.  At 0.9: image 0: d0 tp; d1 (0.8), d5 (0.85) are below the threshold.  Image 1: d2, d4 are below; d3 (0.95) stays
    but overlaps nothing enough and is 24 px high (ignored_det = 1 at every difficulty: no fp); the Car is a fn.  tp 1, fp 0, fn 1.
    At 0.6: image 0: d0 tp; d1 and d5 unassigned -> fp = 2; d1 lies inside the DontCare box (criterion 0: 1 > 0.7) -> nstuff = 1,
    fp = 1.  Image 1: d2 goes to the Van (neither tp nor fp), d4 tp, d3 ignored.  tp 2, fp 1, fn 0.
    precision = [1, 2/3], already non-increasing.  Similarity: d0 alpha 0 -> 1; d4 alpha pi/2 -> (1 + cos(-pi/2)) / 2 = 0.5:
    aos = [1 / 1, 1.5 / 3].
    Ground and 3D metric: the 3D boxes of d0, d2, d4 are their ground truths' (overlap 1), d1, d3, d5 are elsewhere; the DontCare row
    has its 1 x 1 footprint at (-1000, -1000), so d1 stays a fp at 0.6: tp 2, fp 2 -> precision [1, 0.5]."""
    sw, _, (curves,) = ref_eval(pin_b_scene(), [MAIN])
    assert sw.compute_aos
    for d in range(3):
        r = curves[(0, IMAGE, d)]
        assert r.n_gt == 2 and r.thresholds == [0.9, 0.6]
        assert (r.tp, r.fp, r.fn) == ([1, 2], [0, 1], [1, 0])
        assert r.precision[:3] == [1.0, 2.0 / 3.0, 0.0]
        assert r.aos[0] == 1.0 and abs(r.aos[1] - 0.5) <= 1e-15 and r.aos[2] == 0.0
        for m in (GROUND, BOX3D):
            r = curves[(0, m, d)]
            assert r.thresholds == [0.9, 0.6] and (r.tp, r.fp, r.fn) == ([1, 2], [0, 2], [1, 0])
            assert r.precision[:3] == [1.0, 0.5, 0.0] and r.aos is None


def test_pin_c_invalid_alpha_switches_orientation_off():
    scene = pin_b_scene()
    scene[1][1][1].alpha = -10.0                                                 # d3, which is never a true positive
    sw, _, (curves,) = ref_eval(scene, [MAIN])
    assert not sw.compute_aos
    assert all(r.aos is None for r in curves.values())
    assert curves[(0, IMAGE, 0)].precision[:2] == [1.0, 2.0 / 3.0]


def test_pin_max_depth_and_thresholds_count():
    """the distance cut: the Cars stand at 20 m and 30 m; a cut at 25 m ignores the second (n_gt 1), one at 30 m keeps it (t3 > 30 is
    false at 30)"""
    _, _, (near, at) = ref_eval(pin_b_scene(), [grid(25, 0.7), grid(30, 0.7)])
    assert near[(0, IMAGE, 0)].n_gt == 1 and at[(0, IMAGE, 0)].n_gt == 2
    v = [1.0 - k / 400.0 for k in range(300)]
    t = getThresholds(list(v), 300)
    assert len(t) == 41 and t[0] == v[0] and t[-1] == v[-1]


@pytest.mark.parametrize("make, variants, seed", [(scene_mixed, [MAIN, SIDE, grid(30, 0.3), grid(45, 0.5)], 1), (scene_words, [MAIN], 1),
                                                  (scene_many, [MAIN], 1), (scene_rules, [MAIN, SIDE], 1), (scene_no3d, [MAIN], 1)],
                         ids=["mixed", "words", "many", "rules", "no3d"])
def test_committed_seeds_have_margin(make, variants, seed):
    """the seeds the GPU tests use are the first with margin from these starting points: found here, on the CPU"""
    found, scene, (sw, _, curves) = with_margin(make, variants, seed)
    assert found == COMMITTED_SEEDS[make.__name__]
    if make is scene_many:
        r = curves[0][(0, IMAGE, 1)]
        assert len(r.thresholds) == 41 and 250 <= r.n_gt


COMMITTED_SEEDS = {"scene_mixed": 1, "scene_words": 1, "scene_many": 1, "scene_rules": 1, "scene_no3d": 1}


# ---------------------------------------------------------------------------------------------------------------------------
# the package's host side
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    from groomed_nms_amd import _lib
    import groomed_nms_amd
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared in the header" % name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gnms_abi_version() == 1
    assert hasattr(groomed_nms_amd, "kitti_eval") and callable(groomed_nms_amd.run_kitti_eval)
    from groomed_nms_amd import kitti_eval as K
    assert len(K.DISTANCE_GRID) == 28 and K.MAIN == MAIN and K.SIDE == SIDE and K.DISTANCE_GRID[(30, 0.3)] == grid(30, 0.3)
    assert ("#define GNMS_KITTI_EVAL_MAX_DET %d" % K.MAX_DET) in text and ("#define GNMS_KITTI_EVAL_MAX_GT %d" % K.MAX_GT) in text
    assert K.MAX_DET >= 500 and K.MAX_GT >= 64


def _off(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_argument_validation_without_gpu(lib):
    """every check returns -1 before any HIP call"""
    fake = ctypes.c_void_p(256 * 1024)            # never dereferenced on the host
    n = ctypes.c_int64(-1)
    plan = lib.gnms_kitti_eval_plan
    assert plan(_off(0, 2, 5), _off(0, 3, 4), 2, 1, ctypes.byref(n)) == 0 and n.value == 2 * 3 + 3 * 1
    assert plan(None, _off(0, 1), 1, 1, ctypes.byref(n)) == -1 and plan(_off(0, 1), None, 1, 1, ctypes.byref(n)) == -1
    assert plan(_off(0, 1), _off(0, 1), 1, 1, None) == -1
    assert plan(_off(0, 1), _off(0, 1), -1, 1, ctypes.byref(n)) == -1
    assert plan(_off(0, 1), _off(0, 1), 1, 0, ctypes.byref(n)) == -1
    assert plan(_off(0, 3, 2), _off(0, 1, 2), 2, 1, ctypes.byref(n)) == -1 and b"ascending" in lib.gnms_last_error()
    assert plan(_off(0, 1, 2), _off(0, 3, 2), 2, 1, ctypes.byref(n)) == -1
    assert plan(_off(1, 2), _off(0, 1), 1, 1, ctypes.byref(n)) == -1
    assert plan(_off(0, 513), _off(0, 1), 1, 1, ctypes.byref(n)) == -1 and b"limit" in lib.gnms_last_error()
    assert plan(_off(0, 512), _off(0, 1025), 1, 1, ctypes.byref(n)) == -1 and b"limit" in lib.gnms_last_error()
    assert plan(_off(0, 512), _off(0, 1024), 1, 1, ctypes.byref(n)) == 0 and n.value == 512 * 1024
    rec = lib.gnms_kitti_eval_recall
    ok = [fake, fake, fake, fake, fake, 1, 4, 3, 12, fake, fake, 1, fake, fake, fake, fake, fake, None]
    for k in (0, 1, 2, 3, 4, 9, 10, 12, 13, 14, 15, 16):                        # null pointers
        a = list(ok)
        a[k] = None
        assert rec(*a) == -1, k
    for k in (5, 6, 7, 8):                                                      # negative counts
        a = list(ok)
        a[k] = -1
        assert rec(*a) == -1, k
    a = list(ok)
    a[11] = 0
    assert rec(*a) == -1
    pre = lib.gnms_kitti_eval_precision
    ok = [fake, fake, fake, fake, fake, 1, 3, 12, fake, fake, 1] + [fake] * 11 + [None]
    for k in (1, 2, 3, 4, 8, 9) + tuple(range(11, 22)):
        a = list(ok)
        a[k] = None
        assert pre(*a) == -1, k
    for k in (5, 6, 7):
        a = list(ok)
        a[k] = -1
        assert pre(*a) == -1, k


def test_evaluate_rejects_bad_input_before_the_gpu():
    from groomed_nms_amd import kitti_eval as K
    d, g = np.zeros((600, 14)), np.zeros((1, 15))
    with pytest.raises(ValueError, match="limit"):
        K.evaluate(d, np.array([0, 600]), g, np.array([0, 1]))
    with pytest.raises(ValueError, match="ascending"):
        K.evaluate(d[:3], np.array([0, 3, 2, 3]), g, np.array([0, 0, 1, 1]))
    with pytest.raises(ValueError):
        K.evaluate(d[:3], np.array([0, 3]), g, np.array([0, 0, 1]))
    with pytest.raises(ValueError):
        K.evaluate(d[:3], np.array([0, 3]), g, np.array([0, 1]), variants=())


def test_parser_round_trip(tmp_path):
    """files of kitti_io.write_image_boxes_to_txt_file load back to the doubles float() gives for their fields; class names in mixed
    case; a truncated last line is dropped"""
    from groomed_nms_amd import kitti_io, kitti_eval as K
    rng = np.random.default_rng(3)
    conf = {"lbls": ["Car", "pedestrian", "CYCLIST", "Van"]}
    folder = tmp_path / "data"
    folder.mkdir()
    want = []
    for k in range(3):
        n = 4 + k
        boxes = np.zeros((n, 13))
        boxes[:, 0:2] = rng.uniform(0, 500, (n, 2))
        boxes[:, 2:4] = boxes[:, 0:2] + rng.uniform(10, 200, (n, 2))
        boxes[:, 4] = rng.uniform(0, 1, n)
        boxes[:, 5] = rng.integers(1, 5, n)
        boxes[:, 6:9] = rng.uniform(-20, 60, (n, 3))
        boxes[:, 9:12] = rng.uniform(0.5, 4, (n, 3))
        boxes[:, 12] = rng.uniform(-3, 3, n)
        text = kitti_io.write_image_boxes_to_txt_file(boxes, conf, str(folder), "%06d" % k)
        if k == 2:
            with open(folder / ("%06d.txt" % k), "a") as f:
                f.write("Car -1 -1 0.5 10.0 20.0 30.0")                          # a record the file ends in
        rows = []
        for line in text.splitlines():
            f = line.split()
            cid = {"car": 0, "pedestrian": 1, "cyclist": 2}.get(f[0].lower(), -1)
            rows.append([cid] + [float(x) for x in f[3:16]])
        want.append(rows)
    det_rows, off, names = K.load_results(str(folder))
    assert names == ["000000.txt", "000001.txt", "000002.txt"] and off.tolist() == [0, 4, 9, 15] and off.dtype == np.int32
    assert det_rows.dtype == np.float64 and np.array_equal(det_rows, np.array([r for rows in want for r in rows]))
    assert set(det_rows[:, 0]) <= {-1.0, 0.0, 1.0, 2.0} and (det_rows[:, 0] == -1).any() and (det_rows[:, 0] == 2).any()
    # labels: 15 fields, %d occlusion, mixed-case types, a short last line
    lab = tmp_path / "label_2"
    lab.mkdir()
    lines = ["car 0.00 0 -1.57 100.5 120.25 200.75 220.0 1.5 1.6 3.9 1.0 1.5 20.0 -1.6",
             "PERSON_SITTING 0.31 2 0.1 1 2 3 4 1.2 0.5 0.6 -3 1.4 9 0.2",
             "DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10",
             "Tram 0.5 3 1e-1 0 0 10 10 3 2 15 5 1 40 0"]
    for k in range(3):
        with open(lab / ("%06d.txt" % k), "w") as f:
            f.write("\n".join(lines[:k + 2]) + ("\nVan 0.1 1 0.3 5 5" if k == 1 else "\n"))
    gt_rows, goff = K.load_labels(str(lab), names)
    assert goff.tolist() == [0, 2, 5, 9]
    expect = [[{"car": 0, "person_sitting": 4, "dontcare": 5}.get(l.split()[0].lower(), 6)] + [float(x) for x in l.split()[1:]] for l in lines]
    assert np.array_equal(gt_rows, np.array(expect[:2] + expect[:3] + expect[:4]))


def test_ap_and_write_stats(tmp_path):
    from groomed_nms_amd import kitti_io, kitti_eval as K
    rng = np.random.default_rng(0)
    p = rng.uniform(0, 1, (3, 3, 3, 41))
    r40, r11 = K.ap(p, use_40=True), K.ap(p, use_40=False)
    assert r40.shape == r11.shape == (3, 3, 3)
    for idx in np.ndindex(3, 3, 3):
        assert r40[idx] == np.mean(p[idx][1:41]) and r11[idx] == np.mean(p[idx][[0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]])
    result = {"precision": p, "aos": rng.uniform(0, 1, (3, 3, 41)), "compute_aos": True, "eval_image": np.array([True, False, True]),
              "eval_ground": np.array([True, False, False]), "eval_3d": np.array([False, False, True])}
    paths = K.write_stats(result, str(tmp_path), ["Car", "Pedestrian", "Cyclist"])
    assert sorted(os.path.basename(x) for x in paths) == sorted([
        "stats_car_detection.txt", "stats_car_orientation.txt", "stats_car_detection_ground.txt", "stats_cyclist_detection.txt",
        "stats_cyclist_orientation.txt", "stats_cyclist_detection_3d.txt"])
    text = open(tmp_path / "stats_car_detection.txt").read()
    assert text == "".join("".join("%f " % x for x in p[0, 0, d]) + "\n" for d in range(3))
    for use_40 in (True, False):
        rounded = np.array([[float("%f" % x) for x in row] for row in p[0, 1]])
        assert list(kitti_io.parse_kitti_result(str(tmp_path / "stats_car_detection_ground.txt"), use_40=use_40)) == list(K.ap(rounded, use_40=use_40))
        rounded = np.array([[float("%f" % x) for x in row] for row in result["aos"][2]])
        assert list(kitti_io.parse_kitti_result(str(tmp_path / "stats_cyclist_orientation.txt"), use_40=use_40)) == list(K.ap(rounded, use_40=use_40))
    result["compute_aos"] = False
    paths = K.write_stats(result, str(tmp_path), ["Car", "Pedestrian", "Cyclist"])
    assert not os.path.exists(tmp_path / "stats_car_orientation.txt") and len(paths) == 4
