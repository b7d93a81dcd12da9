"""CPU-side tests of the loss module (groomed_nms_amd/loss.py, csrc/loss.hip) and the checkers of its GPU tests.

`restate_gt_filter` is a float64 restatement of lib/loss/rpn_3d.py:399-419 (determine_ignores, rpn_util.py:937-962, bbXYWH2Coords and the
masks) on the packed records; it is checked bit for bit against the igns / rmvs the reference computed and against arrays compacted the
way the reference writes them.  `restate_loss` composes the siblings' restatements (test_sampling_host.restate, the classification term;
test_after_nms_loss_host.restate; test_regression_loss_host.restate) into the reference's total, statistics and the gradients of the
five heads; it is checked against tests/golden/loss.npz (the reference's own RPN_3D_loss.forward and backward with all terms on,
tests/golden/make_loss_golden.py) within max(8 e, 4 float32 ulps), e being the difference the generator recorded for the quantity.
The GPU tests (test_loss_module_gpu.py) hold the module to the restatement."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling_host import restate as restate_sampling  # noqa: E402
from test_regression_loss_host import restate as restate_regression  # noqa: E402
from test_after_nms_loss_host import restate as restate_after_nms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss.npz")
LBLS = ["Car", "Pedestrian", "Cyclist"]
ILBLS = ["Van", "Truck", "Person_sitting", "Tram", "Misc", "DontCare"]
CAPACITY = 64
MODES = ("rank", "rank_all", "classify")
CONFIG_KEYS = ("box_samples", "fg_fraction", "mode", "has_acceptance", "bbox_2d_lambda", "focal_loss", "min_gt_h", "fg_thresh")
# the reference's names in the order of its stats.append calls (:903 to :1407); `after_nms` stands for the mode's name
STAT_KEYS = ("fg", "bg", "cls", "after_nms", "bbox_2d", "cen", "cen_dist_lt_0.2", "axis", "head", "conf", "bbox_3d", "un", "z", "rot", "iou_2d",
             "iou_2d_los", "total")
GRADS = ("grad_cls", "grad_prob", "grad_bbox_2d", "grad_bbox_3d", "grad_acceptance")
E_KEYS = STAT_KEYS + GRADS
AFTER_NAME = {"rank": "bbox_after_nms_rank", "rank_all": "bbox_after_nms_rank", "classify": "bbox_after_nms_class"}
FORMATS = {"fg": ("{:0.2f}", "acc"), "bg": ("{:0.2f}", "acc"), "cls": ("{:0.4f}", "loss"), "after_nms": ("{:0.4f}", "loss"),
           "bbox_2d": ("{:0.4f}", "loss"), "cen": ("{:0.2f}", "misc"), "cen_dist_lt_0.2": ("{:0.3f}", "misc"), "axis": ("{:0.2f}", "acc"),
           "head": ("{:0.2f}", "acc"), "conf": ("{:0.2f}", "misc"), "bbox_3d": ("{:0.4f}", "loss"), "un": ("{:0.4f}", "loss"),
           "z": ("{:0.2f}", "misc"), "rot": ("{:0.2f}", "misc"), "iou_2d": ("{:0.2f}", "acc"), "iou_2d_los": ("{:0.4f}", "loss"),
           "total": ("{:0.4f}", "loss")}
NOT_VERBOSE = ("bg", "bbox_2d", "cen", "axis", "head", "iou_2d_los")       # the entries behind `if self.verbose`


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def conf_of(c, **over):
    """the configuration of a golden case: scripts/config/groumd_nms.py with every term on (the generator runs the reference with it)"""
    acc = bool(c["has_acceptance"])
    return AttrDict(dict(
        lbls=LBLS, ilbls=ILBLS, anchors=c["anchors"], bbox_means=c["means"][None].copy(), bbox_stds=c["stds"][None].copy(), feat_stride=16,
        fg_fraction=c["fg_fraction"], box_samples=c["box_samples"], ign_thresh=0.5, nms_thres=0.4, fg_thresh=c["fg_thresh"], bg_thresh_lo=0.0,
        bg_thresh_hi=0.5, best_thresh=0.35, hard_negatives=True, focal_loss=c["focal_loss"], crop_size=[512, 1760], cls_2d_lambda=1,
        iou_2d_lambda=1, bbox_2d_lambda=c["bbox_2d_lambda"], bbox_3d_lambda=1, bbox_axis_head_lambda=0.35, min_gt_vis=0.65,
        min_gt_h=c["min_gt_h"], max_gt_h=1e9, decomp_alpha=True, has_un=False, predict_acceptance_prob=acc, acceptance_prob_lambda=0,
        acceptance_prob_mode="likelihood", boxes_for_acceptance_prob="foregrounds", use_acceptance_prob_in_regression_loss=acc, bbox_un_lambda=0,
        bbox_un_dynamic=acc, use_nms_in_loss=True, diff_nms_pruning_method="linear", diff_nms_temperature=0.1,
        diff_nms_valid_box_prob_threshold=0.3, diff_nms_boxes_2d="normal", diff_nms_group_boxes=True, diff_nms_mask_group_boxes=True,
        diff_nms_group_size=100, after_nms_lambda=0.05, after_nms_loss_mode="classify" if c["mode"] == "classify" else "rank", overlap_in_nms="2d",
        rank_with_class_confidence=False, rank_boxes_of_all_images_at_once=c["mode"] == "rank_all", best_target_box_beta=0.3), **over)


def records_of(scene, capacity=CAPACITY):
    """the records as pack_ground_truths lays them out, written independently of it: (records [B, capacity, 24], counts [B])"""
    rec = np.zeros((len(scene), capacity, 24))
    counts = np.zeros(len(scene), np.int32)
    for b, gts in enumerate(scene):
        for j, g in enumerate(gts):
            rec[b, j, 0:4] = g["bbox_full"]
            rec[b, j, 4:20] = g["bbox_3d"]
            rec[b, j, 20] = 0 if g["cls"] in ILBLS else (1 + LBLS.index(g["cls"]) if g["cls"] in LBLS else -1)
            rec[b, j, 21:24] = (float(bool(g["ign"])), g.get("visibility", 1.0), g.get("trunc", 0.0))
        counts[b] = len(gts)
    return rec, counts


def restate_gt_filter(records, counts, min_gt_vis, min_gt_h, max_gt_h=10e10, use_trunc=False):
    """:399-419 per image on the records -> dict: igns / rmvs (lists of bool arrays), gts_val [B, cap, 4], box_lbls [B, cap] int32, gts_3d
    [B, cap, 16], gts_ign [B, cap, 4] (zero behind the counts), val_counts, ign_counts"""
    B, cap = records.shape[:2]
    out = dict(igns=[], rmvs=[], gts_val=np.zeros((B, cap, 4)), box_lbls=np.zeros((B, cap), np.int32), gts_3d=np.zeros((B, cap, 16)),
               gts_ign=np.zeros((B, cap, 4)), val_counts=np.zeros(B, np.int32), ign_counts=np.zeros(B, np.int32))
    for b in range(B):
        r = records[b, :max(0, min(int(counts[b]), cap))]
        ign = r[:, 21] != 0                                                    # rpn_util.py:948-952 (scale_factor 1)
        ign = ign | (r[:, 22] < min_gt_vis) | (r[:, 3] < min_gt_h) | (r[:, 3] > max_gt_h) | (r[:, 20] == 0)
        if use_trunc:
            ign = ign | (r[:, 23] > max(1 - min_gt_vis, 0))                    # :954-955
        rmv = r[:, 20] < 0                                                     # :957
        box = r[:, 0:4].copy()                                                 # rpn_util.py:788-789
        box[:, 2] += box[:, 0] - 1
        box[:, 3] += box[:, 1] - 1
        val, keep = ~rmv & ~ign, ~rmv & ign                                    # :410-416
        nv, ni = int(val.sum()), int(keep.sum())
        out["gts_val"][b, :nv], out["gts_3d"][b, :nv], out["box_lbls"][b, :nv] = box[val], r[val, 4:20], r[val, 20].astype(np.int32)
        out["gts_ign"][b, :ni] = box[keep]
        out["val_counts"][b], out["ign_counts"][b] = nv, ni
        out["igns"].append(ign)
        out["rmvs"].append(rmv)
    return out


def restate_loss(c, state_in=(0.0, 0.0), upstream=1.0):
    """the reference's forward and backward on a case's arrays (c: a dict as golden() builds it), composed from the three siblings'
    restatements in float64 -> dict: total, stats (STAT_KEYS -> value), the five gradients, state_out, gt (restate_gt_filter's), sample"""
    gt = restate_gt_filter(c["records"], c["counts"], 0.65, c["min_gt_h"])
    B = c["prob"].shape[0]
    s = restate_sampling(c["transforms"][:, :, 4], c["prob"], gt["val_counts"], c["cls"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"],
                         focal_loss=c["focal_loss"], cls_2d_lambda=1)
    acc = c["acceptance"] if c["has_acceptance"] else None
    rois, r3, cen = (np.ascontiguousarray(np.broadcast_to(c[k][None], (B,) + c[k].shape)) for k in ("rois", "rois_3d", "rois_3d_cen"))
    a = restate_after_nms(c["prob"], acc, c["bbox_2d"], c["bbox_3d"], c["raw_gt"], s["fg_lists"], s["counts"][:, 2], rois, r3, cen, c["p2"],
                          c["scale_factor"], gt["gts_val"], gt["gts_3d"], gt["val_counts"], means=c["means"], stds=c["stds"], after_nms_lambda=0.05,
                          mode=c["mode"], temperature=0.1)
    r = restate_regression(c["bbox_2d"], c["bbox_3d"], acc, c["transforms"], c["raw_gt"], rois, r3, cen, c["p2"], c["scale_factor"], s["fg_lists"],
                           s["counts"][:, 2], means=c["means"], stds=c["stds"], bbox_2d_lambda=c["bbox_2d_lambda"], bbox_3d_lambda=1.0,
                           bbox_axis_head_lambda=0.35, iou_2d_lambda=1.0, use_acceptance=acc is not None, bbox_un_lambda=0.0,
                           bbox_un_dynamic=acc is not None, state_in=state_in)
    st = dict(r["stats"])
    reg = [st[k] for k in ("bbox_2d", "bbox_3d", "un", "iou_2d_los")] if r["n"] else [0.0] * 4
    total = s["loss"] + a["loss"] + sum(reg)                                   # :999, :1138, :1190, :1371, :1380, :1403
    st.update(fg=s["acc_fg"], bg=s["acc_bg"], cls=s["loss"], after_nms=a["loss"], total=total)
    ga = None
    if acc is not None:
        ga = r["grad_acceptance"] + a["grad_acceptance"]
    gp = a["grad_prob"] if a["grad_prob"] is not None else np.zeros(c["prob"].shape)
    out = dict(total=total, stats={k: float(st[k]) for k in STAT_KEYS}, grad_cls=s["grad"], grad_prob=gp, grad_bbox_2d=r["grad_bbox_2d"],
               grad_bbox_3d=r["grad_bbox_3d"], grad_acceptance=ga, state_out=r["state_out"], gt=gt, sample=s, n_active=r["n"], after=a)
    if upstream != 1.0:
        for k in GRADS:
            out[k] = out[k] * upstream if out[k] is not None else None
    return out


# ---------------------------------------------------------------------------------------------- the golden

@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        parts = key.split("/")
        if len(parts) == 3 and not parts[1].startswith("scene_"):
            cases.setdefault((parts[0], parts[1]), {})[parts[2]] = z[key]
    for (shape, _), c in cases.items():
        for k in ("cls", "prob", "bbox_2d", "bbox_3d", "acceptance", "rois", "rois_3d", "rois_3d_cen", "anchors", "p2", "scale_factor", "means", "stds"):
            c[k] = z["%s/%s" % (shape, k)]
        scene = str(c["scene"])
        for k in ("records", "counts", "igns", "rmvs", "transforms", "raw_gt"):
            c[k] = z["%s/scene_%s/%s" % (shape, scene, k)]
        cfg = dict(zip(CONFIG_KEYS, (float(v) for v in c["config"])))
        cfg["mode"], cfg["has_acceptance"] = MODES[int(cfg["mode"])], bool(cfg["has_acceptance"])
        c.update(cfg)
        c["stat_names"] = [str(n) for n in c["stat_names"]]
    return cases


def case_ids():
    return sorted("%s/%s" % k for k in golden()) if os.path.exists(GOLDEN) else []


def case_of(cid):
    return golden()[tuple(cid.split("/"))]


@functools.lru_cache(maxsize=None)
def restated(cid):
    return restate_loss(case_of(cid))


def reference_values(c):
    """-> {key of E_KEYS: the reference's value (a stat it omitted: None)}"""
    names = {AFTER_NAME[c["mode"]]: "after_nms"}
    ref = {k: None for k in STAT_KEYS}
    for n, v in zip(c["stat_names"], c["stat_vals"]):
        ref[names.get(n, n)] = float(v)
    for k in GRADS:
        ref[k] = c[k]
    return ref


def errors_of(c, r):
    """|reference - restatement| per quantity of E_KEYS (the largest entry of a gradient; 0 for a stat the reference omitted)"""
    ref, e = reference_values(c), {}
    for k in STAT_KEYS:
        e[k] = abs(ref[k] - r["stats"][k]) if ref[k] is not None else 0.0
    for k in GRADS:
        e[k] = float(np.abs(ref[k].astype(np.float64) - r[k]).max()) if r[k] is not None else float(np.abs(ref[k]).max())
    return e


def stored_errors(cid):
    return dict(zip(E_KEYS, (float(v) for v in case_of(cid)["e"])))


R210_CASES = {"reference", "classify", "rank_all", "no_acceptance", "with_2d", "focal", "no_gt_image", "all_ignored_image", "mixed"}


def test_golden_holds_the_cases():
    ids = case_ids()
    assert {i.split("/")[1] for i in ids if i.startswith("r210/")} == R210_CASES and "cap/cap" in ids
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert case_of("r210/reference")["bbox_2d"].shape == (2, 210, 4) and case_of("cap/cap")["cls"].shape == (2, 1920, 4)
    n = [len(f) for f in restated("cap/cap")["sample"]["fg_lists"]]
    assert n[0] > 500 > n[1] > 0, n
    assert restated("r210/no_gt_image")["gt"]["val_counts"].tolist()[1] == 0 and case_of("r210/no_gt_image")["counts"][1] == 0
    g = restated("r210/all_ignored_image")["gt"]
    assert g["val_counts"][0] == 0 and g["ign_counts"][0] == case_of("r210/all_ignored_image")["counts"][0] > 0
    # the mixed scene takes every branch of determine_ignores
    c = case_of("r210/mixed")
    rec, n0 = c["records"][0], int(c["counts"][0])
    ids0 = rec[:n0, 20]
    assert (ids0 > 0).any() and (ids0 == 0).sum() >= 2 and (ids0 < 0).sum() == 1
    assert (rec[:n0, 22] < 0.65).any() and c["min_gt_h"] > 0 and (rec[:n0, 3] < c["min_gt_h"]).any() and (rec[:n0, 21] != 0).any()
    assert c["rmvs"][0, :n0].sum() == 1 and 0 < c["igns"][0, :n0].sum() < n0
    assert case_of("r210/no_acceptance")["has_acceptance"] is False and case_of("r210/with_2d")["bbox_2d_lambda"] == 1
    assert case_of("r210/focal")["focal_loss"] == 2 and not case_of("r210/reference")["means"][:4].any()


@pytest.mark.parametrize("cid", case_ids())
def test_gt_filter_restatement_bit_for_bit(cid):
    """against the igns / rmvs the reference's determine_ignores returned, and against the arrays of :403-417 built from them"""
    c = case_of(cid)
    g = restate_gt_filter(c["records"], c["counts"], 0.65, c["min_gt_h"])
    for b in range(len(c["counts"])):
        n = int(c["counts"][b])
        ign, rmv = c["igns"][b, :n].astype(bool), c["rmvs"][b, :n].astype(bool)
        assert np.array_equal(g["igns"][b], ign) and np.array_equal(g["rmvs"][b], rmv), (cid, b)
        xywh = c["records"][b, :n, 0:4]
        box = np.stack([xywh[:, 0], xywh[:, 1], xywh[:, 2] + (xywh[:, 0] - 1), xywh[:, 3] + (xywh[:, 1] - 1)], 1)
        val, keep = ~rmv & ~ign, ~rmv & ign
        nv, ni = int(val.sum()), int(keep.sum())
        assert (g["val_counts"][b], g["ign_counts"][b]) == (nv, ni)
        assert np.array_equal(g["gts_val"][b, :nv], box[val]) and not g["gts_val"][b, nv:].any()
        assert np.array_equal(g["gts_ign"][b, :ni], box[keep]) and not g["gts_ign"][b, ni:].any()
        assert np.array_equal(g["gts_3d"][b, :nv], c["records"][b, :n, 4:20][val]) and not g["gts_3d"][b, nv:].any()
        assert np.array_equal(g["box_lbls"][b, :nv], c["records"][b, :n, 20][val].astype(np.int32)) and (g["box_lbls"][b, :nv] > 0).all()


def test_gt_filter_restatement_use_trunc():
    rec = np.zeros((1, 4, 24))
    rec[0, :, 0:4] = (10.0, 20.0, 30.0, 40.0)
    rec[0, :, 20], rec[0, :, 22] = 1, 1.0
    rec[0, :, 23] = (0.0, 0.3, 0.36, 0.9)
    cnt = np.array([4], np.int32)
    assert restate_gt_filter(rec, cnt, 0.65, 0)["val_counts"][0] == 4
    g = restate_gt_filter(rec, cnt, 0.65, 0, use_trunc=True)
    assert g["igns"][0].tolist() == [False, False, True, True] and g["gts_val"][0, 0].tolist() == [10.0, 20.0, 39.0, 59.0]


@pytest.mark.parametrize("cid", case_ids())
def test_composition_matches_the_reference(cid):
    c, r = case_of(cid), restated(cid)
    e, stored, ref = errors_of(c, r), stored_errors(cid), reference_values(c)
    assert abs(float(c["total"]) - ref["total"]) == 0.0
    for k in E_KEYS:
        top = float(np.abs(ref[k]).max()) if k in GRADS else abs(ref[k] or 0.0)
        tol = max(8 * stored[k], 4 * ulp32(top))
        print("%s: %-16s e %.3e stored %.3e tolerance %.3e (magnitude %.3e)" % (cid, k, e[k], stored[k], tol, top))
        assert e[k] <= tol, (cid, k, e[k], tol)
    # the same foreground as the reference: its axis gradient is non-zero exactly on the active anchors
    mine = np.zeros(c["prob"].shape[:2], bool)
    for b, l in enumerate(r["sample"]["fg_lists"]):
        mine[b, l] = True
    assert np.array_equal(c["grad_bbox_3d"][:, :, 8] != 0, mine)
    assert r["state_out"][0] == (1.0 if c["has_acceptance"] else 0.0)


# ---------------------------------------------------------------------------------------------- the module without a GPU

def _module(**over):
    from groomed_nms_amd.loss import RPN_3D_loss
    verbose = over.pop("verbose", True)
    c = dict(case_of("r210/reference")) if case_ids() else dict(anchors=np.zeros((2, 11)), means=np.zeros(13), stds=np.ones(13), fg_fraction=0.2,
                                                                 box_samples=0.2, fg_thresh=0.5, focal_loss=0, bbox_2d_lambda=0, min_gt_h=0,
                                                                 mode="rank", has_acceptance=True)
    return RPN_3D_loss(conf_of(c, **over), verbose=verbose)


@pytest.mark.parametrize("cid", case_ids())
def test_stats_list_names_groups_formats_order(cid):
    """the list for verbose True is the reference's own list of the case (nothing omitted there: every case has foreground)"""
    from groomed_nms_amd.loss import RPN_3D_loss, STATS_LAYOUT
    c = case_of(cid)
    m = RPN_3D_loss(conf_of(c), verbose=True)
    names = [n for n, _ in m.stat_entries()]
    omitted = [n for n in names if n not in c["stat_names"]]
    assert [n for n in names if n not in omitted] == c["stat_names"], (names, c["stat_names"])
    # the entries the reference omits: conf / un without an acceptance head never appear here either (not configured); nothing else
    assert omitted == [], omitted
    vec = np.arange(len(STATS_LAYOUT), dtype=np.float64)
    for entry, (name, key) in zip(m._stats_list(vec), m.stat_entries()):
        assert entry["name"] == name and (entry["format"], entry["group"]) == FORMATS[key] and entry["val"] == STATS_LAYOUT.index(key)
        assert set(entry) == {"name", "val", "format", "group"}
    quiet = [n for n, _ in RPN_3D_loss(conf_of(c), verbose=False).stat_entries()]
    assert quiet == [n for n, k in m.stat_entries() if k not in NOT_VERBOSE]
    assert STATS_LAYOUT[:len(STAT_KEYS)] == STAT_KEYS


def test_stats_list_follows_the_configuration():
    full = [k for _, k in _module().stat_entries()]
    assert full == list(STAT_KEYS)[:4] + ["cen", "cen_dist_lt_0.2", "axis", "head", "conf", "bbox_3d", "un", "z", "rot", "iou_2d", "iou_2d_los", "total"]
    assert [k for _, k in _module(bbox_2d_lambda=1).stat_entries()] == list(STAT_KEYS)
    assert [n for n, _ in _module(after_nms_loss_mode="classify").stat_entries()][3] == "bbox_after_nms_class"
    off = [k for _, k in _module(cls_2d_lambda=0, use_nms_in_loss=False, bbox_3d_lambda=0, iou_2d_lambda=0, bbox_un_dynamic=False).stat_entries()]
    assert off == ["cen", "cen_dist_lt_0.2", "z", "rot", "iou_2d", "total"]


def test_pack_ground_truths_layout_overflow_unknown_class():
    from groomed_nms_amd.loss import pack_ground_truths, GroundTruths, RECORD_COLS
    rng = np.random.default_rng(2)
    mk = lambda cls, **k: AttrDict(dict(cls=cls, ign=False, visibility=1.0, trunc=0.25, bbox_full=rng.uniform(1, 50, 4), bbox_3d=rng.normal(0, 1, 16)), **k)   # noqa: E731
    scene = [[mk("Cyclist"), mk("Van"), mk("Bus"), mk("Car", ign=True, visibility=0.5)], [], [mk("DontCare")]]
    p2 = rng.normal(0, 1, (4, 4))
    imobjs = [AttrDict(gts=g, p2=p2 if b != 1 else p2[:3], scale_factor=0.5 + b) for b, g in enumerate(scene)]
    gt = pack_ground_truths(imobjs, LBLS, ILBLS, capacity=5)
    assert isinstance(gt, GroundTruths) and RECORD_COLS == 24 and gt.records.shape == (3, 5, 24) and gt.records.dtype.is_floating_point
    rec, counts = records_of(scene, 5)
    assert np.array_equal(gt.records.numpy(), rec) and np.array_equal(gt.counts.numpy(), counts) and counts.tolist() == [4, 0, 1]
    assert gt.records[0, :4, 20].tolist() == [3.0, 0.0, -1.0, 1.0] and gt.records[0, 3, 21:24].tolist() == [1.0, 0.5, 0.25]
    assert np.array_equal(gt.p2[0].numpy(), p2) and np.array_equal(gt.p2[1, :3].numpy(), p2[:3]) and gt.p2[1, 3].tolist() == [0, 0, 0, 1]
    assert gt.scale_factor.tolist() == [0.5, 1.5, 2.5]
    # one buffer holds them all, and a copy into kept buffers keeps their addresses
    assert gt.buffer.numel() == GroundTruths.elements(3, 5) and gt.records.data_ptr() == gt.buffer.data_ptr()
    kept = GroundTruths.empty(3, 5, device="cpu")
    where = kept.records.data_ptr()
    assert gt.to("cpu", out=kept) is kept and kept.records.data_ptr() == where and np.array_equal(kept.buffer.numpy(), gt.buffer.numpy())
    assert pack_ground_truths(imobjs, LBLS, ILBLS, key="gts", capacity=4).records.shape == (3, 4, 24)
    with pytest.raises(ValueError, match="capacity"):
        pack_ground_truths(imobjs, LBLS, ILBLS, capacity=3)
    with pytest.raises(ValueError):
        pack_ground_truths(imobjs, LBLS, ILBLS, capacity=257)
    with pytest.raises(ValueError):
        gt.to("cpu", out=GroundTruths.empty(2, 5, device="cpu"))


@pytest.mark.parametrize("key,over", [
    ("has_un", dict(has_un=True)), ("orientation_bins", dict(orientation_bins=4)), ("decomp_alpha", dict(decomp_alpha=False)),
    ("infer_2d_from_3d", dict(infer_2d_from_3d=True)), ("hard_negatives", dict(hard_negatives=False)),
    ("acceptance_prob_lambda", dict(predict_acceptance_prob=True, acceptance_prob_lambda=1.0)),
    ("acceptance_prob_mode", dict(acceptance_prob_mode="classify")), ("overlap_in_nms", dict(overlap_in_nms="3d")),
    ("overlap_in_nms", dict(overlap_in_nms="product")), ("after_nms_loss_mode", dict(after_nms_loss_mode="regress")),
    ("weigh_3D_regression_loss_by_gt_iou3d", dict(weigh_3D_regression_loss_by_gt_iou3d=True)),
    ("boxes_for_acceptance_prob", dict(boxes_for_acceptance_prob="all", after_nms_loss_mode="classify"))])
def test_unsupported_keys_raise_at_construction(key, over):
    with pytest.raises(NotImplementedError, match=key):
        _module(**over)


def test_supported_configurations_construct():
    _module()
    _module(boxes_for_acceptance_prob="all")                     # per-image ranking reads the sampled foreground whatever the key says
    _module(predict_acceptance_prob=True, acceptance_prob_lambda=0, acceptance_prob_mode="likelihood")
    _module(after_nms_loss_mode="regress", use_nms_in_loss=False)
    m = _module(verbose=False)
    assert m.verbose is False and m.un_state is None and m.last_stats is None
    import inspect
    from groomed_nms_amd.loss import RPN_3D_loss
    assert list(inspect.signature(RPN_3D_loss.forward).parameters) == ["self", "cls", "prob", "bbox_2d", "bbox_3d", "imobjs", "feat_size", "rois", "rois_3d",
                                                                       "rois_3d_cen", "bbox_acceptance_prob", "bbox_acceptance_prob_cls", "key"]
    assert list(inspect.signature(RPN_3D_loss.__init__).parameters)[:3] == ["self", "conf", "verbose"]
    with pytest.raises(NotImplementedError, match="bbox_acceptance_prob_cls"):
        m.forward(None, None, None, None, [], [1, 1], bbox_acceptance_prob_cls=object())


def test_abi_symbols_and_argument_errors_without_gpu():
    import ctypes
    from groomed_nms_amd import build, _lib
    import groomed_nms_amd
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    for name in ("gnms_gt_filter", "gnms_loss_combine", "gnms_loss_grad_combine"):
        assert "int %s(" % name in header and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "loss.hip" in build.SOURCES and groomed_nms_amd.RPN_3D_loss is groomed_nms_amd.loss.RPN_3D_loss
    for name, val in re.findall(r"#define (GNMS_LOSS_\w+) (\d+)", header):
        from groomed_nms_amd import loss
        assert {"GNMS_LOSS_RECORD_COLS": loss.RECORD_COLS, "GNMS_LOSS_MAX_GTS": loss.MAX_GTS, "GNMS_LOSS_STATS": len(loss.STATS_LAYOUT)}[name] == int(val)
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)      # never dereferenced on the host
    f = lambda **k: lib.gnms_gt_filter(k.get("rec", fake), fake, k.get("B", 2), k.get("cap", 64), 0.65, 0.0, 1e11, 0, fake, fake, fake,   # noqa: E731
                                       k.get("ign", fake), fake, fake, None)
    assert f(B=0) == 0 and f(B=-1) == -1 and f(cap=0) == -2 and f(cap=257) == -2 and b"256" in lib.gnms_last_error()
    assert f(rec=None) == -1 and f(ign=None) == -1 and f(rec=odd) == -1 and b"aligned" in lib.gnms_last_error()
    assert lib.gnms_loss_combine(fake, fake, fake, fake, fake, None, fake, None) == -1
    assert lib.gnms_loss_combine(fake, None, fake, fake, fake, fake, fake, None) == -1
    assert lib.gnms_loss_combine(fake, fake, fake, fake, None, fake, fake, None) == -1
    g = lambda rows=10, C=4, D3=11, up=fake, out=fake: lib.gnms_loss_grad_combine(up, rows, C, D3, fake, fake, fake, fake, fake, fake, out, fake, fake,   # noqa: E731
                                                                                  fake, fake, None)
    assert g(rows=0) == 0 and g(rows=-1) == -1 and g(up=None) == -1 and g(C=0) == -1 and g(out=odd) == -1 and g(C=65) == -1
    assert lib.gnms_loss_grad_combine(fake, 10, 4, 11, fake, fake, fake, fake, fake, fake, None, None, None, None, None, None) == 0


def test_product_does_not_import_the_checker():
    src = open(os.path.join(ROOT, "groomed_nms_amd", "loss.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("the GPU tests", "")
