"""CPU-side tests of the after-NMS block of the RPN loss (groomed_nms_amd/after_nms.py, csrc/after_nms.hip, the tail of csrc/aploss.hip).

`restate` below is the checker: a NumPy restatement of lib/loss/rpn_3d.py:721-825 and :1091-1148 from the heads, with the reference's
line numbers.  The decode of the selected anchors (:316-363, :532-574) is float64 on the float32 inputs; the layer, the best box per
ground truth and the AP loss are the oracle's (oracle/oracle.py, oracle/proposals_oracle.py) as they are.  It is checked here against
tests/golden/after_nms.npz (the reference's own RPN_3D_loss.forward and backward, tests/golden/make_after_nms_golden.py): index sets,
target sets and img_cnt exactly, and per golden case e_ref = |reference - restatement| of the loss, the statistic and each gradient
(largest entry), which the GPU tests (test_after_nms_loss_gpu.py) take from here.  The sampled foreground comes from
test_sampling_host.restate (the sampler's checker).
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling_host import restate as restate_sampling  # noqa: E402
from test_regression_loss_host import snap_to_pi, decode_2d, _ctype_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
import oracle.proposals_oracle as PO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "after_nms.npz")
PRUNE = ("linear", "sigmoidal", "soft_nms")
MODES = ("rank", "rank_all", "classify")
CONFIG_KEYS = ("box_samples", "fg_fraction", "after_nms_lambda", "mode", "rank_with_class_confidence", "has_acceptance", "projected",
               "pruning", "group_boxes", "mask_group_boxes", "group_size", "best_target_box_beta", "nms_threshold", "temperature",
               "valid_box_prob_threshold", "max_nms_boxes")
f32 = np.float32


def decode_selected(bbox_2d, bbox_3d, raw_gt, rois, rois_3d, cen, p2, scale, means, stds, sel):
    """:316 and :318-363, :532-574 for the anchors `sel` of one image, float64 on the float32 inputs -> (boxes [n, 4], cuboids [n, 7])"""
    d2, b3, gt = bbox_2d[sel].astype(np.float64), bbox_3d[sel].astype(np.float64), raw_gt[sel].astype(np.float64)
    roi, r3, c = rois[sel].astype(np.float64), rois_3d[sel].astype(np.float64), cen[sel].astype(np.float64)
    w, h = roi[:, 2] - roi[:, 0] + 1.0, roi[:, 3] - roi[:, 1] + 1.0                       # :338-339
    boxes, _, _ = decode_2d(d2, means, stds, w, h, roi[:, 0] + 0.5 * w, roi[:, 1] + 0.5 * h)
    dn = lambda k, col: b3[:, col] * stds[k] + means[k]                                   # noqa: E731  (:318-328)
    x_dn, y_dn = dn(4, 0) * w + c[:, 0], dn(5, 1) * h + c[:, 1]                           # :351-352
    z_dn = r3[:, 4] + dn(6, 2)                                                            # :354
    with np.errstate(all="ignore"):
        whl = [np.exp(dn(7 + k, 3 + k)) * r3[:, 5 + k] for k in range(3)]                 # :355-357
    rsin, rcos = r3[:, 9] + dn(11, 6), r3[:, 10] + dn(12, 7)                              # :362-363
    P = np.asarray(p2, np.float64)
    z_raw = z_dn - P[2, 3]                                                                # :553
    x_raw = ((z_raw + P[2, 3]) * (x_dn / scale) - P[0, 2] * z_raw - P[0, 3]) / P[0, 0]   # :554
    y_raw = ((z_raw + P[2, 3]) * (y_dn / scale) - P[1, 2] * z_raw - P[1, 3]) / P[1, 1]   # :555
    rot = np.where(gt[:, 19] == 1.0, rsin, rcos)                                          # :569-570
    rot = np.where(gt[:, 20] == 1.0, rot + np.pi, rot)                                    # :571
    ry = snap_to_pi(snap_to_pi(rot) + np.arctan2(-z_raw, x_raw) + 0.5 * np.pi)            # :573-574, util.py:635-638
    return boxes, np.stack([x_raw, y_raw, z_raw] + whl + [ry], 1)


def projected_f64(cuboids, p2, scale):
    """:746-768 in float64"""
    c = O.corners_of_cuboid_numpy_branch(cuboids)                                         # [n, 3, 8]
    P = np.eye(4)
    P[:np.asarray(p2).shape[0]] = p2
    pts = np.concatenate([c, np.ones((len(c), 1, 8))], 1)                                 # [n, 4, 8]
    q = np.einsum("ij,njk->nik", P, pts)
    ok = np.abs(q[:, 2]) > 1e-2                                                           # math_3d.py:56, :64
    xy = np.where(ok[:, None], q[:, :2] / np.where(ok, q[:, 2], 1.0)[:, None], q[:, :2])
    return np.stack([xy[:, 0].min(1), xy[:, 1].min(1), xy[:, 0].max(1), xy[:, 1].max(1)], 1) * scale


def bce_clamped(p, y):
    """F.binary_cross_entropy (logs clamped at -100) and its derivative (denominator clamped at 1e-12)"""
    with np.errstate(all="ignore"):
        lp, lq = np.log(p), np.log(1.0 - p)
    lp, lq = np.where(lp < -100.0, -100.0, lp), np.where(lq < -100.0, -100.0, lq)
    den = (1.0 - p) * p
    with np.errstate(all="ignore"):
        return (y - 1.0) * lq - y * lp, (p - y) / np.where(den > 1e-12, den, 1e-12)


def restate(prob, acceptance, bbox_2d, bbox_3d, raw_gt, fg_lists, fg_num, rois, rois_3d, rois_3d_cen, p2, scale_factor, gts_val, gts_3d,
            val_counts, *, means, stds, after_nms_lambda=0.05, mode="rank", rank_with_class_confidence=False, best_target_box_beta=0.3,
            nms_threshold=0.4, pruning_method="linear", temperature=0.1, valid_box_prob_threshold=0.3, group_boxes=True,
            mask_group_boxes=True, group_size=100, projected=False, max_nms_boxes=500, tail=True, upstream=1.0):
    """-> dict: loss, losses [B], img_cnt, sel / scores / prob / targets / tails (lists per image, selection order), iou (the float64
    overlaps), score_gt (the [n, M] scores with the ground truths), grad_acceptance [B, R] or None, grad_prob [B, R, C] or None.
    tail=False leaves out the sampled foreground beyond the selected boxes (what ranking only the NMS's boxes would give)."""
    B, R = bbox_2d.shape[:2]
    means, stds = np.asarray(means, np.float64), np.asarray(stds, np.float64)
    use_prob = acceptance is None or rank_with_class_confidence
    layer = dict(nms_threshold=nms_threshold, pruning_method=pruning_method, temperature=temperature,
                 valid_box_prob_threshold=valid_box_prob_threshold, return_sorted_prob=False, group_boxes=group_boxes,
                 mask_group_boxes=mask_group_boxes, group_size=group_size)
    out = dict(sel=[], scores=[], prob=[], targets=[], tails=[], iou=[], score_gt=[], nms_iou32=[])
    amax = None
    if use_prob:
        amax = prob[:, :, 1:].argmax(2) + 1
        pmax = np.take_along_axis(prob, amax[:, :, None], 2)[:, :, 0].astype(f32)
        scores_all = pmax * acceptance.astype(f32) if acceptance is not None else pmax     # :722-727, one fp32 product
    else:
        scores_all = acceptance.astype(f32)
    for b in range(B):
        fg = np.asarray(fg_lists[b], np.int64)
        sel = PO.select_topk(scores_all[b], fg, max_nms_boxes) if (fg_num[b] > 0 and len(fg)) else np.zeros(0, np.int64)   # :729-737
        n = len(sel)
        s = scores_all[b][sel]
        p, t, iou, sg, iou32 = np.zeros(0, f32), np.zeros(0, f32), np.zeros((0, 0)), np.zeros((0, 0), f32), np.zeros((0, 0), f32)
        if n:
            boxes, cub = decode_selected(bbox_2d[b], bbox_3d[b], raw_gt[b], rois[b], rois_3d[b], rois_3d_cen[b], p2[b], float(scale_factor[b]),
                                         means, stds, sel)
            nb = projected_f64(cub, p2[b], float(scale_factor[b])) if projected else boxes
            iou = O.iou2d_f64(nb, nb)                                                      # :772-774
            iou32 = O.iou2d(nb.astype(f32), nb.astype(f32))
            p = O.differentiable_nms(s, iou32, **layer)["prob"]                            # :791
            m = int(val_counts[b])
            gp = gts_3d[b][:m][:, [7, 8, 9, 3, 4, 5, 10]].astype(f32)                      # :805-811
            gb = gts_val[b][:m].astype(f32)
            t = np.zeros(n, f32)
            if m:
                t, _, _ = PO.best_targets(cub.astype(f32), boxes.astype(f32), gp, gb, best_target_box_beta)               # :813-825
                pc, gc = O.corners_of_cuboid(cub.astype(f32)), O.corners_of_cuboid(gp)
                sg = (f32(0.5) * (f32(1.0) + O.iou3d_approximate(pc, gc, generalized=True)[1])) * O.iou2d(boxes.astype(f32), gb)
        for k, v in (("sel", sel), ("scores", s), ("prob", p), ("targets", np.asarray(t, f32)), ("tails", (len(fg) - n) if tail else 0),
                     ("iou", iou), ("score_gt", sg), ("nms_iou32", iou32)):
            out[k].append(v)
    fg_counts = np.array([len(f) for f in fg_lists])
    img_cnt = int((fg_counts > 0).sum())
    lam = float(after_nms_lambda)
    dprob = [np.zeros(len(s), f32) for s in out["sel"]]
    losses = np.zeros(B)
    if fg_counts.sum() == 0:                                                               # :1100-1101
        loss = 0.0
    elif mode == "classify":                                                               # :1103-1115
        p = np.concatenate(out["prob"]).astype(np.float64)
        y = np.concatenate(out["targets"]).astype(np.float64)
        E = int(sum(out["tails"]))
        npos, nneg = int((y == 1).sum()), int((y == 0).sum()) + E
        w = np.ones(len(p))
        if npos > 0 and nneg > 0:
            w[y == 0] = float(f32(np.power(npos / nneg, 0.25)))
        v, dv = bce_clamped(p, y)
        fin = np.isfinite(w * v)
        nfin = int(fin.sum()) + E
        loss = lam * float((w * v)[fin].sum()) / nfin if nfin else np.nan
        g = np.where(fin, lam * w * dv / max(nfin, 1), 0.0)
        off = 0
        for b in range(B):
            dprob[b] = g[off:off + len(out["sel"][b])].astype(f32)
            off += len(out["sel"][b])
    elif mode == "rank_all":                                                               # :1119
        E = int(sum(out["tails"]))
        lg = np.concatenate(out["prob"] + [np.zeros(E, f32)])
        tg = np.concatenate(out["targets"] + [np.zeros(E, f32)])
        l, g = O.aploss(lg, tg)
        loss = lam * l
        off = 0
        for b in range(B):
            dprob[b] = (g[off:off + len(out["sel"][b])] * f32(lam)).astype(f32)
            off += len(out["sel"][b])
    else:                                                                                  # :1121-1131
        total = 0.0
        for b in range(B):
            if fg_counts[b] > 0:
                E = out["tails"][b]
                l, g = O.aploss(np.concatenate([out["prob"][b], np.zeros(E, f32)]), np.concatenate([out["targets"][b], np.zeros(E, f32)]))
                losses[b] = l
                total += l
                dprob[b] = (g[:len(out["sel"][b])].astype(np.float64) * lam / img_cnt).astype(f32)
        loss = lam * total / img_cnt
    ga = np.zeros((B, R)) if acceptance is not None else None
    gpr = np.zeros(prob.shape) if use_prob else None
    for b in range(B):
        sel = out["sel"][b]
        if not len(sel):
            continue
        ds = O.differentiable_nms(out["scores"][b], out["nms_iou32"][b], grad_prob=dprob[b], **layer)["grad_scores"].astype(np.float64) * upstream
        if use_prob:
            cls = amax[b][sel]
            if ga is not None:
                ga[b, sel] = ds * prob[b, sel, cls].astype(np.float64)
            gpr[b, sel, cls] = ds * (acceptance[b, sel].astype(np.float64) if acceptance is not None else 1.0)
        else:
            ga[b, sel] = ds
    out.update(loss=float(loss), losses=losses, img_cnt=img_cnt, grad_acceptance=ga, grad_prob=gpr, fg_counts=fg_counts)
    return out


# ---------------------------------------------------------------------------------------------- the goldens

def kw_of(config):
    c = dict(zip(CONFIG_KEYS, (float(v) for v in config)))
    return dict(after_nms_lambda=c["after_nms_lambda"], mode=MODES[int(c["mode"])], rank_with_class_confidence=bool(c["rank_with_class_confidence"]),
                best_target_box_beta=c["best_target_box_beta"], nms_threshold=c["nms_threshold"], pruning_method=PRUNE[int(c["pruning"])],
                temperature=c["temperature"], valid_box_prob_threshold=c["valid_box_prob_threshold"], group_boxes=bool(c["group_boxes"]),
                mask_group_boxes=bool(c["mask_group_boxes"]), group_size=int(c["group_size"]), projected=bool(c["projected"]),
                max_nms_boxes=int(c["max_nms_boxes"]))


def api_kw(kw):
    """the restatement's keywords -> after_nms_loss's"""
    k = dict(kw)
    mode = k.pop("mode")
    k["after_nms_loss_mode"] = "classify" if mode == "classify" else "rank"
    k["rank_boxes_of_all_images_at_once"] = mode == "rank_all"
    k["diff_nms_boxes_2d"] = "projected" if k.pop("projected") else "normal"
    return k


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        parts = key.split("/")
        if len(parts) == 3 and not parts[1].startswith("scene_"):
            cases.setdefault((parts[0], parts[1]), {})[parts[2]] = z[key]
    for (shape, _), c in cases.items():
        for k in ("prob", "bbox_2d", "bbox_3d", "acceptance", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor", "means", "stds"):
            c[k] = z["%s/%s" % (shape, k)]
        for k in ("rois", "rois_3d", "rois_3d_cen"):                    # one anchor grid for both images
            c[k] = np.ascontiguousarray(np.broadcast_to(c[k][None], (2,) + c[k].shape))
        scene = str(c["scene"])
        for k in ("raw_gt", "target_labels", "val_counts", "gts_val", "gts_3d"):
            c[k] = z["%s/scene_%s/%s" % (shape, scene, k)]
        cfg = dict(zip(CONFIG_KEYS, (float(v) for v in c["config"])))
        c["box_samples"], c["fg_fraction"] = cfg["box_samples"], cfg["fg_fraction"]
        c["kw"] = kw_of(c["config"])
        if not cfg["has_acceptance"]:
            c["acceptance"] = None
    return cases


def case_ids():
    return sorted("%s/%s" % k for k in golden())


def case_of(cid):
    return golden()[tuple(cid.split("/"))]


@functools.lru_cache(maxsize=None)
def sampled(cid):
    c = case_of(cid)
    return restate_sampling(c["target_labels"], c["prob"], c["val_counts"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])


def restate_case(c, s, **over):
    return restate(c["prob"], c["acceptance"], c["bbox_2d"], c["bbox_3d"], c["raw_gt"], s["fg_lists"], s["counts"][:, 2], c["rois"], c["rois_3d"],
                   c["rois_3d_cen"], c["p2"], c["scale_factor"], c["gts_val"], c["gts_3d"], c["val_counts"], means=c["means"], stds=c["stds"],
                   **dict(c["kw"], **over))


@functools.lru_cache(maxsize=None)
def restated(cid):
    return restate_case(case_of(cid), sampled(cid))


@functools.lru_cache(maxsize=None)
def reference_errors(cid):
    """e_ref of a golden case: |reference - restatement| of the loss, the statistic and each gradient (largest entry)"""
    c, r = case_of(cid), restated(cid)
    e = {"loss": abs(float(c["loss"]) - r["loss"]), "stat": abs(float(c["stat"]) - r["loss"])}
    for k in ("grad_acceptance", "grad_prob"):
        e[k] = float(np.abs(c[k].astype(np.float64) - r[k]).max()) if r[k] is not None else float(np.abs(c[k]).max())
    return e


R210_CASES = {"reference", "rank_all", "classify", "class_confidence", "no_acceptance", "projected", "sigmoidal", "soft_nms", "groups_off",
              "groups_no_mask", "no_gt_image", "all_ignored_image", "quota_zero", "high_beta"}


def test_golden_holds_the_cases():
    ids = case_ids()
    assert {i.split("/")[1] for i in ids if i.startswith("r210/")} == R210_CASES
    assert "cap/cap" in ids
    assert os.path.getsize(GOLDEN) < 1 << 20
    c, s = case_of("cap/cap"), sampled("cap/cap")
    n = [len(f) for f in s["fg_lists"]]
    assert n[0] > 500 > n[1] > 0, n                          # image 0 is cut to the 500 best and carries a zero tail, image 1 is not
    r = restated("cap/cap")
    assert len(r["sel"][0]) == 500 and r["tails"][0] == n[0] - 500 and r["tails"][1] == 0
    assert sampled("r210/quota_zero")["counts"][:, 2].tolist() == [0, 0] and restated("r210/quota_zero")["img_cnt"] == 2
    assert sampled("r210/no_gt_image")["counts"][1].sum() == 0 and restated("r210/no_gt_image")["img_cnt"] == 1
    hb = restated("r210/high_beta")
    assert min(float(t.sum()) for t in hb["targets"]) == 0 and max(float(t.sum()) for t in hb["targets"]) > 0
    assert case_of("r210/no_acceptance")["acceptance"] is None


@pytest.mark.parametrize("cid", case_ids() if os.path.exists(GOLDEN) else [])
def test_restatement_matches_the_reference(cid):
    c, r = case_of(cid), restated(cid)
    B = c["bbox_2d"].shape[0]
    assert r["img_cnt"] == int(c["img_cnt"])
    for b in range(B):
        # the reference's selection (the scores that went into the layer identify the anchors: no two foreground scores are equal)
        assert np.array_equal(r["scores"][b], c["nms_scores_%d" % b]), (cid, b)
        assert np.array_equal(r["sel"][b], c["sel_%d" % b]), (cid, b)
        assert np.array_equal(np.sort(r["sel"][b][r["targets"][b] == 1]), c["target_index_%d" % b]), (cid, b)
    e = reference_errors(cid)
    scale = {"loss": abs(float(c["loss"])), "grad_acceptance": float(np.abs(c["grad_acceptance"]).max()), "grad_prob": float(np.abs(c["grad_prob"]).max())}
    print("%s: loss %.9g (reference %.9g); e_ref %s; magnitudes %s" % (cid, r["loss"], float(c["loss"]), e, scale))
    # the restatement's layer, AP loss and best targets are fp32 oracles pinned bit for bit elsewhere; what remains between it and the
    # reference is the fp32 decode in front of them and the order of the AP loss's additions (anchor order there, selection order
    # here): a few hundred roundings at most
    assert e["loss"] <= 1024 * 2.0 ** -24 * max(abs(float(c["loss"])), float(c["kw"]["after_nms_lambda"]))
    for k in ("grad_acceptance", "grad_prob"):
        assert e[k] <= 4096 * 2.0 ** -24 * max(scale[k], 1e-30) or scale[k] == 0.0 and e[k] == 0.0, (k, e[k], scale[k])


def test_the_cap_case_tells_the_tail_apart():
    """on the cap case the restatement WITHOUT the zero tail must miss the reference by more than 100 e_ref"""
    c, e = case_of("cap/cap"), reference_errors("cap/cap")
    r = restate_case(c, sampled("cap/cap"), tail=False)
    miss = abs(r["loss"] - float(c["loss"]))
    gmiss = float(np.abs(r["grad_acceptance"] - c["grad_acceptance"]).max())
    print("cap: e_ref loss %.3g, without the tail the loss misses by %.3g; gradient e_ref %.3g, miss %.3g" % (e["loss"], miss, e["grad_acceptance"], gmiss))
    assert miss > 100 * e["loss"] and miss > 0
    assert gmiss > 100 * e["grad_acceptance"]


def test_restatement_edge_rules():
    """the rules the goldens cannot isolate, on a hand-made batch: ties at the cut, the window of the tail, an empty batch"""
    rng = np.random.default_rng(5)
    B, R, M = 2, 12, 2
    c = case_of("r210/reference")
    args = dict(means=c["means"], stds=c["stds"])
    take = lambda a: a[:, :R]            # noqa: E731
    acc = take(c["acceptance"]).copy()
    acc[0, 3] = acc[0, 5]                                                  # a tie: the lower anchor index goes first
    fg = [np.array([1, 3, 5, 7]), np.zeros(0, np.int64)]
    base = (take(c["prob"]), acc, take(c["bbox_2d"]), take(c["bbox_3d"]), take(c["raw_gt"]))
    rest = (take(c["rois"]), take(c["rois_3d"]), take(c["rois_3d_cen"]), c["p2"], c["scale_factor"], c["gts_val"][:, :M], c["gts_3d"][:, :M],
            np.array([M, 0]))
    r = restate(*base, fg, np.array([4, 0]), *rest, max_nms_boxes=3, **args)
    s = acc[0][r["sel"][0]]
    assert len(r["sel"][0]) == 3 and r["tails"] == [1, 0] and r["img_cnt"] == 1 and (np.diff(s) <= 0).all()
    if 3 in r["sel"][0] and 5 in r["sel"][0]:
        assert list(r["sel"][0]).index(3) < list(r["sel"][0]).index(5)
    e = restate(*base, [np.zeros(0, np.int64)] * 2, np.array([0, 0]), *rest, **args)
    assert e["loss"] == 0.0 and e["img_cnt"] == 0 and not e["grad_acceptance"].any()
    q = restate(*base, fg, np.array([0, 0]), *rest, **args)               # quota 0: counted, contributes 0
    assert q["loss"] == 0.0 and q["img_cnt"] == 1 and q["tails"] == [4, 0] and not q["grad_acceptance"].any()
    del rng


# ---------------------------------------------------------------------------------------------- the library's surface, without a GPU

NEW_SYMBOLS = ("gnms_aploss_tail", "gnms_after_nms_decode", "gnms_after_nms_finish", "gnms_after_nms_scatter")


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def test_abi_symbols_and_prototypes(lib):
    from groomed_nms_amd import _lib, build
    assert "after_nms.hip" in build.SOURCES
    text = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\bint\s+%s\s*\(([^;{}]*)\)\s*;" % name, text)
        assert m, "%s is not declared in the header" % name
        args = [_ctype_of(a) for a in m.group(1).split(",")]
        assert _lib._SIGNATURES[name] == (ctypes.c_int, args), "%s: the ctypes prototype and the header disagree" % name
    assert lib.gnms_abi_version() == 1


def test_argument_errors_without_gpu(lib):
    """every check below returns before a HIP call"""
    INVALID, UNSUPPORTED = -1, -2
    fake = ctypes.c_void_p(1 << 20)
    v = (ctypes.c_double * 13)(*([1.0] * 13))
    host = ctypes.cast(v, ctypes.c_void_p)

    def decode(B=2, K=8, R=64, D3=11, ld_gt=21, ld_rois=5, ld_r3=11, p2_rows=4, ld_g3=16, M=3, null=None):
        p = [fake] * 19
        if null is not None:
            p[null] = None
        return lib.gnms_after_nms_decode(p[0], p[1], B, K, R, p[2], p[3], D3, p[4], ld_gt, p[5], ld_rois, p[6], ld_r3, p[7], p[8], p2_rows, p[9],
                                         host, host, p[10], p[11], ld_g3, M, p[12], p[13], p[14], p[15], p[16], None)
    assert decode(K=0) == INVALID and decode(R=0) == INVALID and decode(M=0) == INVALID and decode(B=-1) == INVALID
    assert decode(D3=9) == INVALID and decode(ld_gt=20) == INVALID and decode(ld_rois=3) == INVALID and decode(ld_r3=10) == INVALID
    assert decode(ld_g3=10) == INVALID and decode(p2_rows=2) == INVALID and b"p2" in lib.gnms_last_error()
    for k in range(17):
        assert decode(null=k) == INVALID, k
    assert decode(B=0) == 0
    tail = lambda N=64, tc=fake, B=2: lib.gnms_aploss_tail(fake, fake, B, N, None, tc, 1.0, 0.0, fake, fake, None)      # noqa: E731
    assert tail(N=4097) == UNSUPPORTED and b"4096" in lib.gnms_last_error()
    assert tail(tc=None) == INVALID and tail(N=-1) == INVALID and tail(B=0) == 0
    fin = lambda phase=1, mode=0, B=2, K=8, M=3, null=(): lib.gnms_after_nms_finish(phase, mode, B, K, *[None if i in null else fake for i in range(6)], 0.05,      # noqa: E731
                                                                               *[None if 6 + i in null else fake for i in range(5)],
                                                                               None if 11 in null else fake, M, None)
    assert fin(phase=2) == INVALID and fin(mode=3) == INVALID and fin(K=0) == INVALID and fin(B=1 << 30, K=4) == INVALID
    assert fin(phase=0, null=(11,)) == INVALID and fin(phase=0, M=0) == INVALID and fin(phase=0, null=(6,)) == INVALID and fin(phase=0, null=(7,)) == INVALID and fin(phase=1, null=(8,)) == INVALID
    assert fin(phase=1, null=(4,)) == INVALID and fin(phase=1, mode=2, null=(2,)) == INVALID and fin(null=(0,)) == INVALID
    sc = lambda B=2, K=8, R=64, C=4, acc=fake, prob=None, cls=None, dacc=fake, dprob=None, ds=fake: lib.gnms_after_nms_scatter(      # noqa: E731
        fake, fake, ds, B, K, R, C, acc, prob, cls, dacc, dprob, None)
    assert sc(K=0) == INVALID and sc(R=0) == INVALID and sc(dacc=None) == INVALID and sc(acc=None, dacc=None) == INVALID
    assert sc(prob=fake) == INVALID and sc(prob=fake, dprob=fake) == INVALID and sc(prob=fake, dprob=fake, cls=fake, C=1) == INVALID
    assert sc(ds=None) == INVALID and sc(B=0) == 0


def test_module_surface_and_host_errors():
    import collections
    import torch
    import groomed_nms_amd
    from groomed_nms_amd import after_nms
    assert groomed_nms_amd.after_nms_loss is after_nms.after_nms_loss and "after_nms_loss" in after_nms.__all__
    assert "after_nms" in groomed_nms_amd.__doc__
    assert after_nms.STAT_NAME == {"rank": "bbox_after_nms_rank", "classify": "bbox_after_nms_class"}
    B, R, M = 2, 8, 3
    S = collections.namedtuple("S", ["fg_index", "fg_counts", "counts"])
    s = S(torch.zeros((B, R), dtype=torch.int32), torch.zeros(B, dtype=torch.int32), torch.zeros((B, 6), dtype=torch.int32))
    z = lambda *shape: torch.zeros(shape)      # noqa: E731
    good = dict(prob=z(B, R, 4), acceptance=z(B, R), bbox_2d=z(B, R, 4), bbox_3d=z(B, R, 11), targets=(z(B, R, 14), z(B, R, 21)), sample=s,
                rois=z(B, R, 5), rois_3d=z(B, R, 11), rois_3d_cen=z(B, R, 2), p2=z(B, 4, 4), scale_factor=z(B), gts_val=z(B, M, 4),
                gts_3d=z(B, M, 16), val_counts=torch.zeros(B, dtype=torch.int32), means=[0.0] * 13, stds=[1.0] * 13)
    for kw in (dict(after_nms_loss_mode="regress"), dict(overlap_in_nms="3d"), dict(overlap_in_nms="product"), dict(decomp_alpha=False),
               dict(pruning_method="other")):
        with pytest.raises(NotImplementedError):
            after_nms.after_nms_loss(**good, **kw)
    with pytest.raises(ValueError, match="GPU"):                  # CPU tensors never reach the library
        after_nms.after_nms_loss(**good)
    with pytest.raises(ValueError, match="int32"):
        after_nms.after_nms_loss(**dict(good, sample=S(s.fg_index.long(), s.fg_counts, s.counts)))
    with pytest.raises(ValueError, match="4096"):
        after_nms.after_nms_loss(**good, rank_boxes_of_all_images_at_once=True, max_nms_boxes=4000)
    for key, bad in (("bbox_2d", z(B, R, 5)), ("bbox_3d", z(B, R, 9)), ("acceptance", z(B, R, 1)), ("targets", (z(B, R, 14), z(B, R, 20))),
                     ("rois", z(B, R, 3)), ("rois_3d", z(1, R, 11)), ("rois_3d_cen", z(B, R, 1)), ("means", [0.0] * 12), ("p2", z(B, 2, 4)),
                     ("scale_factor", z(B + 1)), ("gts_val", z(B, M, 5)), ("gts_3d", z(B, M, 10)), ("gts_3d", z(B, M + 1, 16)),
                     ("val_counts", torch.zeros(B + 1, dtype=torch.int32)), ("max_nms_boxes", 0), ("diff_nms_boxes_2d", "other"),
                     ("sample", S(torch.zeros((B, R + 1), dtype=torch.int32), s.fg_counts, s.counts))):
        with pytest.raises(ValueError):
            after_nms.after_nms_loss(**dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="prob"):
        after_nms.after_nms_loss(**dict(good, prob=z(B, R, 1)), rank_with_class_confidence=True)
    with pytest.raises(ValueError):
        after_nms.after_nms_loss(**dict(good, prob=None, acceptance=None))
