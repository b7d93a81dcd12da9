"""Generate tests/golden/targets.npz by IMPORTING the reference's compute_targets (lib/rpn_util.py:411-524) and iou_ign
(lib/core.py:535-575).  Runs only where the reference checkout is (REF below, read-only); it writes data only: each case's
inputs and the reference's outputs, keyed 'case/field'.  The reference checkout (abhi1kumar/groomed_nms) is the first argument.

The reference's lib/rpn_util.py imports cv2, torchvision, PIL, lib.augmentations and the compiled lib.nms.gpu_nms at module top;
none of them is used by compute_targets, so they are stubbed.  usage: python tests/golden/make_targets_golden.py REFERENCE_CHECKOUT"""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "targets.npz")


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
    import lib.core as core           # noqa: E402
    return rpn_util, core


THRESH = dict(fg=0.5, ign=0.5, lo=0.0, hi=0.5, best=0.35)        # scripts/config/groumd_nms.py


def anchor_grid(rng, H=6, W=16, A=6, stride=16, dtype=np.float32):
    """rois [H*W*A, 5] (x1 y1 x2 y2 tracker) like locate_anchors (anchor-major per cell), and the anchors [A, 4] they come from"""
    wh = np.stack([rng.uniform(16, 90, A), rng.uniform(16, 70, A)], 1)
    anchors = np.concatenate([-wh / 2, wh / 2], 1)
    ys, xs = np.meshgrid(np.arange(H) * stride, np.arange(W) * stride, indexing="ij")
    shifts = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], 1).astype(np.float64)
    rois = (shifts[:, None, :] + anchors[None]).reshape(-1, 4)
    tracker = np.tile(np.arange(A), H * W).astype(np.float64)
    return np.concatenate([rois, tracker[:, None]], 1).astype(dtype), anchors


def anchors_3d(rng, a2d, cols):
    A = a2d.shape[0]
    out = np.zeros((A, cols))
    out[:, :4] = a2d
    out[:, 4] = rng.uniform(5, 40, A)                       # z
    out[:, 5:8] = rng.uniform(0.5, 4, (A, 3))               # w h l
    out[:, 8] = rng.uniform(-3, 3, A)                       # ry
    if cols >= 11:
        out[:, 9] = np.sin(out[:, 8])
        out[:, 10] = np.cos(out[:, 8])
    if cols == 12:
        out[:, 11] = rng.uniform(-2, 2, A)
    return out


def gts_near(rng, rois, n, jitter=6.0):
    pick = rng.choice(len(rois), n, replace=False)
    g = rois[pick, :4].astype(np.float64) + rng.normal(0, jitter, (n, 4))
    g[:, 2:] = np.maximum(g[:, 2:], g[:, :2] + 4)
    return g


def gts3d(rng, M, D3):
    g = np.zeros((M, D3))
    g[:, 0:2] = rng.uniform(0, 256, (M, 2))
    g[:, 2] = rng.uniform(5, 50, M)
    g[:, 3:6] = rng.uniform(0.5, 4, (M, 3))
    g[:, 6:] = rng.uniform(-3, 3, (M, D3 - 6))
    return g


def rois_3d_of(rng, rois, anchors, cols):
    r3 = np.zeros((len(rois), cols), np.float32)
    r3[:, :4] = rois[:, :4]
    src = anchors[rois[:, 4].astype(np.int64)]
    r3[:, 4:min(cols, anchors.shape[1])] = src[:, 4:cols] + rng.normal(0, 0.05, (len(rois), min(cols, anchors.shape[1]) - 4))
    return r3


def main():
    if not REF:
        sys.exit(__doc__)
    rpn_util, core = load_reference()
    rng = np.random.default_rng(2026)
    z = {}

    def case(name, gts_val, gts_ign, lbls, rois, th=THRESH, gts_3d=None, anchors=None, rois_3d=None, rois_3d_cen=None, use_tracker=False,
             norm=None):
        kw = {}
        if gts_3d is not None:
            kw["gts_3d"] = gts_3d
        kw["anchors"] = anchors if anchors is not None else np.zeros((1, 9))       # 2D-only: anchors.shape[1] = 9 is "neither"
        if gts_3d is not None:                                 # read whenever there are 3D targets (:475)
            kw["tracker"] = rois[:, 4]
        if rois_3d is not None:
            kw["rois_3d"] = rois_3d
        if rois_3d_cen is not None:
            kw["rois_3d_cen"] = rois_3d_cen
        t, o, g = rpn_util.compute_targets(gts_val, gts_ign, lbls, rois, th["fg"], th["ign"], th["lo"], th["hi"], th["best"], **kw)
        p = name + "/"
        z[p + "gts_val"] = np.asarray(gts_val, np.float64).reshape(-1, 4)
        z[p + "gts_ign"] = np.asarray(gts_ign, np.float64).reshape(-1, 4)
        z[p + "box_lbls"] = np.asarray(lbls, np.int64)
        z[p + "rois"] = rois
        z[p + "thresh"] = np.array([th["fg"], th["ign"], th["lo"], th["hi"], th["best"]])
        if gts_3d is not None:
            z[p + "gts_3d"] = gts_3d
        if anchors is not None:
            z[p + "anchors"] = anchors
        if rois_3d is not None:
            z[p + "rois_3d"] = rois_3d
        if rois_3d_cen is not None:
            z[p + "rois_3d_cen"] = rois_3d_cen
        z[p + "use_tracker"] = np.array(use_tracker)
        z[p + "transforms"] = t
        z[p + "raw_gt"] = g
        if o is not None:
            z[p + "ols"] = o
        if len(gts_ign):
            z[p + "ols_ign"] = core.iou_ign(rois, np.asarray(gts_ign, np.float64))
        if norm is not None:                                   # lib/loss/rpn_3d.py:440-451 on the reference's output
            means, stds = norm
            tn = t.copy()
            tn[:, 0:4] -= means[:, 0:4]
            tn[:, 0:4] /= stds[:, 0:4]
            if t.shape[1] == 5:                                # 2D only: columns 0:4
                pass
            elif anchors is not None and anchors.shape[1] >= 11:
                tn[:, 5:14] -= means[:, 4:13]
                tn[:, 5:14] /= stds[:, 4:13]
            else:
                tn[:, 5:12] -= means[:, 4:11]
                tn[:, 5:12] /= stds[:, 4:11]
            z[p + "means"] = means
            z[p + "stds"] = stds
            z[p + "transforms_norm"] = tn

    def lbls(M):
        return rng.integers(1, 4, M)

    # the loss call site (rpn_3d.py:435): float32 rois, rois_3d + centre, decomp_alpha, D3 = 16, normalised as :440-451
    rois, a2 = anchor_grid(rng)
    an = anchors_3d(rng, a2, 11)
    r3 = rois_3d_of(rng, rois, an, 11)
    cen = ((rois[:, :2] + rois[:, 2:4]) / 2 + rng.normal(0, 1, (len(rois), 2))).astype(np.float32)
    gv = gts_near(rng, rois, 12)
    means = rng.normal(0, 0.1, (1, 13))
    stds = rng.uniform(0.1, 2, (1, 13))
    case("loss", gv, gts_near(rng, rois, 4, 20), lbls(12), rois, gts_3d=gts3d(rng, 12, 16), anchors=an, rois_3d=r3, rois_3d_cen=cen,
         norm=(means, stds))
    # the statistics pass (rpn_util.py:620-699): float64 rois, anchors[tracker], no centre
    rois64, a2 = anchor_grid(rng, dtype=np.float64)
    an = anchors_3d(rng, a2, 11)
    case("stats", gts_near(rng, rois64, 10), gts_near(rng, rois64, 2, 20), lbls(10), rois64, gts_3d=gts3d(rng, 10, 16), anchors=an,
         use_tracker=True)
    # 2D only (rpn_util.py:626), without decomp: normalisation of columns 0:4 only
    case("2d", gts_near(rng, rois, 8), gts_near(rng, rois, 3, 20), lbls(8), rois,
         norm=(rng.normal(0, 0.1, (1, 11)), rng.uniform(0.1, 2, (1, 11))))
    # 3D without decomp (anchors of 9 columns): the 5:12 normalisation
    an9 = anchors_3d(rng, a2, 9)
    case("nodecomp", gts_near(rng, rois, 8), np.zeros((0, 4)), lbls(8), rois, gts_3d=gts3d(rng, 8, 16), anchors=an9,
         rois_3d=rois_3d_of(rng, rois, an9, 9), norm=(rng.normal(0, 0.1, (1, 11)), rng.uniform(0.1, 2, (1, 11))))
    # has_vel: D3 = 16 (delta_vel = -inf) and D3 = 17
    an12 = anchors_3d(rng, a2, 12)
    case("vel16", gts_near(rng, rois, 8), gts_near(rng, rois, 2), lbls(8), rois, gts_3d=gts3d(rng, 8, 16), anchors=an12,
         rois_3d=rois_3d_of(rng, rois, an12, 12), rois_3d_cen=cen)
    case("vel17", gts_near(rng, rois, 8), gts_near(rng, rois, 2), lbls(8), rois, gts_3d=gts3d(rng, 8, 17), anchors=an12,
         rois_3d=rois_3d_of(rng, rois, an12, 12), rois_3d_cen=cen)
    case("vel17_anchors", gts_near(rng, rois64, 8), np.zeros((0, 4)), lbls(8), rois64, gts_3d=gts3d(rng, 8, 17), anchors=an12,
         use_tracker=True)
    # only ignore boxes (M = 0), with and without 3D; nothing at all
    case("ign_only", np.zeros((0, 4)), gts_near(rng, rois, 3, 15), np.zeros(0, np.int64), rois)
    case("ign_only_3d", np.zeros((0, 4)), gts_near(rng, rois, 3, 15), np.zeros(0, np.int64), rois, gts_3d=np.zeros((0, 16)), anchors=an,
         rois_3d=r3)
    case("empty", np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(0, np.int64), rois, th=dict(THRESH, lo=0.1))
    # no ignore boxes, and ign_thresh <= 0 (every roi ignored through the zero ols_ign_max)
    case("no_ign", gts_near(rng, rois, 6), np.zeros((0, 4)), lbls(6), rois)
    case("no_ign_thresh0", gts_near(rng, rois, 6), np.zeros((0, 4)), lbls(6), rois, th=dict(THRESH, ign=0.0))
    # duplicate GTs and duplicate rois: first-argmax ties both ways
    rd = rois.copy()
    rd[7] = rd[3]
    rd[100] = rd[3]
    rd[101] = rd[40]
    g = gts_near(rng, rd, 5)
    g = np.concatenate([g, g[1:2], g[3:4], rd[3:4, :4].astype(np.float64), rd[3:4, :4].astype(np.float64)])
    case("dups", g, gts_near(rng, rd, 2, 20), np.array([1, 2, 3, 1, 2, 3, 1, 3, 2]), rd)
    # a GT whose best roi lies below fg but above best, and two GTs sharing one best roi (with different labels)
    gb = np.array([100.0, 40.0, 300.0, 52.0])                  # 200 x 12: no anchor covers it well
    gs1 = rois[200, :4].astype(np.float64) + np.array([-1.0, 0, -1.0, 0])
    gs2 = rois[200, :4].astype(np.float64) + np.array([1.0, 0, 1.0, 0])
    case("best_below_fg", np.stack([gb, gs1, gs2]), np.zeros((0, 4)), np.array([2, 1, 3]), rois, th=dict(THRESH, fg=0.7, best=0.2))
    # best_thresh = 0 and a GT that overlaps nothing: its best roi is roi 0
    far = np.array([[5000.0, 5000.0, 5050.0, 5040.0]])
    case("best0", np.concatenate([gts_near(rng, rois, 3), far]), np.zeros((0, 4)), np.array([1, 2, 3, 2]), rois, th=dict(THRESH, best=0.0))
    # zero-area rois (NaN in iou_ign, ols 0) and a degenerate GT
    rz = rois.copy()
    rz[3, 2] = rz[3, 0]
    rz[9, 3] = rz[9, 1]
    gz = gts_near(rng, rz, 4)
    gi = np.concatenate([rz[3:4, :4], rz[9:10, :4] + np.array([-5, -5, 5, 5], np.float32)]).astype(np.float64)
    case("zero_area", gz, gi, lbls(4), rz)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
