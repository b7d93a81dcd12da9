"""Generate tests/golden/kitti_rows.npz by IMPORTING the reference's validation tail and running it on prepared detections: per image
the slice and the threshold of lib/train_test.py:102-107, convert_image_predictions_to_correct_entries and
get_text_to_write_in_kitti_format (lib/rpn_util.py:1489-1631).  The text is then split into tokens and every numeric token parsed with
float(), which is what the devkit's fscanf("%lf") reads.  Runs only where the reference checkout is (first argument, read-only); it
writes data only: each case's inputs, the text of every image and the parsed rows, keyed 'case/field'.

Stubbed: the modules lib/rpn_util.py imports at its top and does not use on this path (the stub modules of make_targets_golden.py).

Guard band, asserted here: a case is redrawn (new seed, at most 20 times, the number is stored) until
  * no field's unrounded float64 value lies within 1e-9 of a decimal tie (k + 1/2) 1e-6,
  * no angle that enters a snap_to_pi lies within 1e-9 of +-pi,
  * no score lies within 1e-9 of score_thres, except the one placed on it exactly (it must be dropped: the comparison is strict).
Inside that band a last-ulp difference between NumPy's matmul / arctan2 and another implementation cannot change a printed digit, a
wrap or a keep decision, so the stored rows can be demanded exactly.

usage: python tests/golden/make_kitti_rows_golden.py REFERENCE_CHECKOUT"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_targets_golden import _Stub  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "kitti_rows.npz")
BAND, MAX_REDRAWS = 1e-9, 20
CLASS_IDS = {"car": 0, "pedestrian": 1, "cyclist": 2}


def load_reference():
    for name in ("cv2", "torchvision", "torchvision.transforms", "easydict", "shapely", "shapely.geometry", "visdom",
                 "lib.augmentations", "lib.nms", "lib.nms.gpu_nms"):
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules["lib.nms.gpu_nms"].gpu_nms = None
    sys.path.insert(0, REF)
    import lib.rpn_util as rpn_util   # noqa: E402
    return rpn_util


class Conf(dict):
    __getattr__ = dict.__getitem__


# name -> B, Kmax, counts, nms_topN_post, score_thres, lbls, share of scores above the threshold, image whose rows are all dropped
CASES = [
    # a wave boundary inside an image, the cut (70 -> 50), an empty first image, a fourth class that maps to -1
    ("wave_boundary", 3, 70, [0, 70, 37], 50, 0.75, ["Car", "Pedestrian", "Cyclist", "Van"], 0.5, None),
    # more rows than one pass of a workgroup (256): kept rows on both sides of row 256; an image without a kept row in the middle
    ("two_passes", 4, 300, [300, 20, 0, 11], 290, 0.5, ["car", "Cyclist", "PEDESTRIAN"], 0.08, 1),
]


def make_inputs(rng, B, Kmax, counts, thres, n_lbls, share, dropped):
    f32 = np.float32
    det = np.zeros((B, Kmax, 14), f32)
    x1 = rng.uniform(0, 1100, (B, Kmax))
    y1 = rng.uniform(0, 300, (B, Kmax))
    det[..., 0], det[..., 1] = x1, y1
    det[..., 2], det[..., 3] = x1 + rng.uniform(5, 200, (B, Kmax)), y1 + rng.uniform(5, 120, (B, Kmax))
    above = rng.random((B, Kmax)) < share                              # kept and dropped rows interleave
    above[B - 1] = rng.random(Kmax) < 0.5                              # (the last image appends behind whatever the others left)
    det[..., 4] = np.where(above, rng.uniform(thres + 1e-3, 1.0, (B, Kmax)), rng.uniform(0.0, thres - 1e-3, (B, Kmax)))
    det[..., 5] = rng.integers(1, n_lbls + 1, (B, Kmax))
    det[..., 6] = rng.uniform(-100, 1350, (B, Kmax))                   # u, v: the projected centre (left of the principal point: x < 0)
    det[..., 7] = rng.uniform(100, 300, (B, Kmax))
    det[..., 8] = rng.uniform(2, 70, (B, Kmax))
    det[..., 9] = rng.uniform(0.4, 2.2, (B, Kmax))
    det[..., 10] = rng.uniform(1.2, 2.1, (B, Kmax))
    det[..., 11] = rng.uniform(0.5, 5.0, (B, Kmax))
    det[..., 12] = rng.uniform(-4.5, 4.5, (B, Kmax))                   # alpha + atan2(-z, x) + pi / 2 leaves (-pi, pi] on both sides
    det[..., 13] = rng.integers(0, 36, (B, Kmax))
    if dropped is not None:
        det[dropped, :, 4] = rng.uniform(0.0, thres - 1e-3, Kmax)
    exact = None
    for b in range(B):                                                 # one score on the threshold itself, among the rows that take part
        if counts[b] >= 4 and b != dropped:
            exact = (b, 3)
            det[b, 3, 4] = f32(thres)
            assert float(det[b, 3, 4]) == thres
            break
    assert exact is not None
    # rows behind an image's count keep their random contents (high scores among them): they must not be read
    p2 = np.zeros((B, 4, 4))
    for b in range(B):
        f = rng.uniform(700, 730)
        p2[b] = [[f, 0, rng.uniform(590, 620), rng.uniform(30, 60)], [0, f, rng.uniform(165, 185), rng.uniform(-1, 1)],
                 [0, 0, 1, rng.uniform(0.001, 0.005)], [0, 0, 0, 1]]
    return det, p2, exact


def near_tie(v):
    s = np.abs(np.asarray(v, np.float64)) * 1e6
    return np.abs(s - np.floor(s) - 0.5) < BAND * 1e6


def near_pi(a):
    a = np.abs(np.asarray(a, np.float64))
    k = np.round((a - math.pi) / (2 * math.pi))                        # the loops compare with +-pi after every step of 2 pi
    return np.abs(a - math.pi - k * 2 * math.pi) < BAND


def run_case(rpn_util, seed, B, Kmax, counts, topn, thres, lbls, share, dropped):
    rng = np.random.default_rng(seed)
    det, p2, exact = make_inputs(rng, B, Kmax, counts, thres, len(lbls), share, dropped)
    conf = Conf(lbls=lbls, score_thres=thres, nms_topN_post=topn)
    ok = True
    texts, rows, offsets = [], [], [0]
    for b in range(B):
        aboxes = det[b, :counts[b]].astype(np.float64)                 # im_detect_3d returns float64 (lib/rpn_util.py:1338-1356)
        aboxes = aboxes[:min(conf.nms_topN_post, aboxes.shape[0])]     # lib/train_test.py:102-107
        scores_img = aboxes[:, 4]
        for k in range(len(scores_img)):
            if abs(scores_img[k] - thres) < BAND and (b, k) != exact:
                ok = False
        gt_thresh_indices = np.where(scores_img > conf.score_thres)[0]
        assert not (exact[0] == b and exact[1] in gt_thresh_indices)
        aboxes = aboxes[gt_thresh_indices]
        boxes_image = rpn_util.convert_image_predictions_to_correct_entries(aboxes, conf, p2[b])
        text = rpn_util.get_text_to_write_in_kitti_format(boxes_image, conf)
        # the band, on the unrounded values the text was printed from
        x, z, ry = boxes_image[:, 6], boxes_image[:, 8], boxes_image[:, 12]
        az = np.arctan2(-z, x)
        first = aboxes[:, 12] + az + 0.5 * math.pi
        second = ry - az - 0.5 * math.pi
        alpha = rpn_util.convertRot2Alpha(ry.copy(), z, x)
        fields = np.column_stack([alpha, boxes_image[:, 0:5], boxes_image[:, 6:13]]) if len(aboxes) else np.zeros((0, 13))
        ok &= not near_tie(fields).any() and not near_pi(first).any() and not near_pi(second).any()
        for line in text.splitlines():
            tok = line.split()
            assert len(tok) == 16 and tok[1] == "-1" and tok[2] == "-1"
            rows.append([float(CLASS_IDS.get(tok[0].lower(), -1))] + [float(t) for t in tok[3:]])
        offsets.append(len(rows))
        texts.append(text)
        if dropped == b:
            assert counts[b] > 0 and text == ""
    rows = np.array(rows, np.float64).reshape(-1, 14)
    return ok, dict(det=det, counts=np.array(counts, np.int32), p2=p2, score_thres=np.array(thres), nms_topN_post=np.array(topn),
                    lbls=np.array(lbls), rows=rows, offsets=np.array(offsets, np.int32), text=np.array(texts), exact=np.array(exact))


def check_coverage(name, d):
    """the properties the cases are there for"""
    rows, off = d["rows"], d["offsets"]
    assert (rows[:, 9] < 0).any() and (rows[:, 9] > 0).any(), "boxes on both sides of the camera axis"
    det, counts, topn, thres = d["det"], d["counts"], int(d["nms_topN_post"]), float(d["score_thres"])
    wrapped_hi = wrapped_lo = 0
    for b in range(len(counts)):
        m = min(int(counts[b]), topn)
        keep = det[b, :m, 4].astype(np.float64) > thres
        assert keep.sum() == off[b + 1] - off[b]
        if m > 2 and keep.any():
            assert not keep.all() and np.abs(np.diff(keep.astype(int))).sum() >= 2, "kept and dropped rows interleave"
        a = det[b, :m, 12].astype(np.float64)[keep]
        r = rows[off[b]:off[b + 1]]
        first = a + np.arctan2(-r[:, 11], r[:, 9]) + 0.5 * math.pi
        wrapped_hi += int((first > math.pi).sum())
        wrapped_lo += int((first <= -math.pi).sum())
    assert wrapped_hi and wrapped_lo, "angles on both sides of +-pi"
    if name == "wave_boundary":
        assert (rows[:, 0] == -1).any() and set(rows[:, 0]) == {-1.0, 0.0, 1.0, 2.0}
        assert counts[1] > topn and (det[1, topn:counts[1], 4] > thres).any(), "the cut drops rows the threshold would keep"
    if name == "two_passes":
        assert off[1] > 0 and off[2] == off[1] and off[3] == off[2] and off[4] > off[3], "rows behind an image that kept none"
        keep = det[0, :topn, 4].astype(np.float64) > thres
        assert keep[:64].any() and keep[64:128].any() and keep[128:256].any() and keep[256:].any(), "kept rows in several waves and both passes"


def main():
    if not REF:
        sys.exit(__doc__)
    rpn_util = load_reference()
    z = {}
    for ci, (name, B, Kmax, counts, topn, thres, lbls, share, dropped) in enumerate(CASES):
        for redraw in range(MAX_REDRAWS + 1):
            ok, d = run_case(rpn_util, 7000 + 100 * ci + redraw, B, Kmax, counts, topn, thres, lbls, share, dropped)
            if ok:
                break
        else:
            sys.exit("case %s needs more than %d redraws" % (name, MAX_REDRAWS))
        check_coverage(name, d)
        for k, v in d.items():
            z[name + "/" + k] = v
        z[name + "/redraws"] = np.array(redraw)
        print("%-16s B=%d Kmax=%d redraws=%d rows=%d offsets=%s" % (name, B, Kmax, redraw, len(d["rows"]), d["offsets"].tolist()))
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
