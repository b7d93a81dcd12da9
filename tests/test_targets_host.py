"""Anchor target assignment (compute_targets, csrc/targets.hip) without a GPU: a NumPy restatement of the contract that matches the
reference's goldens (tests/golden/targets.npz) bit for bit, the C symbols are declared, bound and exported, and argument validation
answers before anything touches a device.

The checker is written from the contract, not from the reference's code: roi-only terms in the rois' dtype, every
term with a ground truth in float64, NumPy's NaN rules for max / argmax."""
import os

import numpy as np
import pytest

from conftest import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inter(r, g):
    """[R, G] float64 intersection areas of rois r [R, >=4] (any float dtype) and boxes g [G, 4] float64"""
    r = r[:, :4].astype(np.float64)
    iw = np.clip(np.minimum(r[:, None, 2], g[None, :, 2]) - np.maximum(r[:, None, 0], g[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(r[:, None, 3], g[None, :, 3]) - np.maximum(r[:, None, 1], g[None, :, 1]), 0, None)
    return iw * ih


def _area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def ign_matrix(rois, gts_ign):
    """iou_ign: inter / (area_roi + area_ign * 0 - inter * 0), area_roi in the rois' dtype"""
    inter = _inter(rois, gts_ign)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((_area(rois[:, :4]).astype(np.float64)[:, None] + (_area(gts_ign) * 0.0)[None]) - inter * 0.0)


def checker(gts_val, gts_ign, box_lbls, rois, fg, ign, lo, hi, best, gts_3d=None, anchors=None, rois_3d=None, rois_3d_cen=None,
            tracker=None, means=None, stds=None):
    """the contract for one image -> dict(transforms, raw_gt, ols, ols_max, best_roi)"""
    rois = np.asarray(rois)
    T = rois.dtype.type
    R = rois.shape[0]
    gts_val = np.asarray(gts_val, np.float64).reshape(-1, 4)
    gts_ign = np.asarray(gts_ign, np.float64).reshape(-1, 4)
    M, K = len(gts_val), len(gts_ign)
    ac = 0 if anchors is None else anchors.shape[1]
    decomp, vel = ac >= 11, ac == 12
    D3 = gts_3d.shape[1] if gts_3d is not None else 0
    Wt = 5 + D3 + 2 * decomp + vel if gts_3d is not None else 5
    Wr = 5 + D3 if gts_3d is not None else 5
    t = np.zeros((R, Wt), np.float32)
    g = np.zeros((R, Wr), np.float32)
    ols = None
    ols_max = np.zeros(R)
    best_roi = np.full(M, -1, np.int64)
    if M == 0 and K == 0:
        t[:, 4] = -1
    else:
        im = ign_matrix(rois, gts_ign).max(axis=1) if K else np.zeros(R)
        fg_mask = np.zeros(R, bool)
        if M:
            inter = _inter(rois, gts_val)
            with np.errstate(invalid="ignore", divide="ignore"):
                ols = inter / ((_area(rois[:, :4]).astype(np.float64)[:, None] + _area(gts_val)[None]) - inter)
            ols_max = ols.max(axis=1)
            tgt = ols.argmax(axis=1)
            b_idx, b_val = ols.argmax(axis=0), ols.max(axis=0)
            kept = b_val >= best
            best_roi[kept] = b_idx[kept]
            fg_mask = ols_max >= fg
            fg_mask[b_idx[kept]] = True
            f = np.flatnonzero(fg_mask)
            j = tgt[f]
            x1, y1, x2, y2 = (rois[f, c] for c in range(4))
            ew, eh = x2 - x1 + T(1.0), y2 - y1 + T(1.0)
            ecx, ecy = x1 + T(0.5) * ew, y1 + T(0.5) * eh
            gv = gts_val[j]
            gw, gh = gv[:, 2] - gv[:, 0] + 1.0, gv[:, 3] - gv[:, 1] + 1.0
            gcx, gcy = gv[:, 0] + 0.5 * gw, gv[:, 1] + 0.5 * gh
            ewd, ehd = ew.astype(np.float64), eh.astype(np.float64)
            t[f, 0] = (gcx - ecx) / ewd
            t[f, 1] = (gcy - ecy) / ehd
            t[f, 2] = np.log(gw / ewd)
            t[f, 3] = np.log(gh / ehd)
            t[f, 4] = np.asarray(box_lbls)[j]
            g[f, 0:4] = gv
            if gts_3d is not None:
                g3 = gts_3d[j]
                if rois_3d is not None:
                    s = rois_3d[f, 4:]
                else:
                    s = anchors[np.asarray(tracker).astype(np.int64)[f], 4:]
                cx = rois_3d_cen[f, 0] if rois_3d_cen is not None else ecx
                cy = rois_3d_cen[f, 1] if rois_3d_cen is not None else ecy
                cols = [(g3[:, 0] - cx) / ewd, (g3[:, 1] - cy) / ehd, g3[:, 2] - s[:, 0], np.log(g3[:, 3] / s[:, 1]),
                        np.log(g3[:, 4] / s[:, 2]), np.log(g3[:, 5] / s[:, 3]), g3[:, 6] - s[:, 4]]
                if decomp:
                    cols += [g3[:, 12] - s[:, 5], g3[:, 13] - s[:, 6]]
                    if vel:
                        cols.append(g3[:, 16] - s[:, 7] if D3 == 17 else np.full(len(f), -np.inf))
                cols += [g3[:, k] for k in range(7, D3)]
                for c, v in enumerate(cols):
                    t[f, 5 + c] = v
                g[f, 5:] = g3
        bg = (ols_max >= lo) & (ols_max < hi) & ~(im >= ign) & ~fg_mask
        t[bg, 4] = -1
    if means is not None:
        n3 = (9 if decomp else 7) if gts_3d is not None else 0
        cols = list(range(4)) + list(range(5, 5 + n3))
        for i, c in enumerate(cols):
            t[:, c] = (t[:, c].astype(np.float64) - means.reshape(-1)[i]).astype(np.float32)
            t[:, c] = (t[:, c].astype(np.float64) / stds.reshape(-1)[i]).astype(np.float32)
    return dict(transforms=t, raw_gt=g, ols=ols, ols_max=ols_max, best_roi=best_roi)


def case_inputs(z, c):
    """the golden case's arguments for checker() / compute_targets()"""
    p = c + "/"
    th = z[p + "thresh"]
    kw = dict(gts_3d=z[p + "gts_3d"] if z.has(p + "gts_3d") else None, anchors=z[p + "anchors"] if z.has(p + "anchors") else None,
              rois_3d=z[p + "rois_3d"] if z.has(p + "rois_3d") else None, rois_3d_cen=z[p + "rois_3d_cen"] if z.has(p + "rois_3d_cen") else None)
    if kw["gts_3d"] is not None:
        kw["tracker"] = z[p + "rois"][:, 4]
    return (z[p + "gts_val"], z[p + "gts_ign"], z[p + "box_lbls"], z[p + "rois"], *[float(v) for v in th]), kw


@pytest.fixture(scope="module")
def gold():
    return Golden("targets.npz")


def same(a, b):
    return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_golden_covers_the_contract(gold):
    cases = set(gold.cases())
    assert {"loss", "stats", "2d", "vel16", "vel17", "ign_only", "no_ign", "empty", "dups", "best_below_fg", "best0", "zero_area"} <= cases
    assert np.isinf(gold["vel16/transforms"]).any() and not np.isinf(gold["vel17/transforms"]).any()
    assert np.isnan(gold["zero_area/ols_ign"]).any()
    assert (gold["empty/transforms"][:, 4] == -1).all()
    assert gold["loss/rois"].dtype == np.float32 and gold["stats/rois"].dtype == np.float64


@pytest.mark.parametrize("case", ["loss", "stats", "2d", "nodecomp", "vel16", "vel17", "vel17_anchors", "ign_only", "ign_only_3d", "empty",
                                  "no_ign", "no_ign_thresh0", "dups", "best_below_fg", "best0", "zero_area"])
def test_checker_matches_reference_bit_for_bit(gold, case):
    args, kw = case_inputs(gold, case)
    r = checker(*args, **kw)
    assert same(r["transforms"], gold[case + "/transforms"])
    assert same(r["raw_gt"], gold[case + "/raw_gt"])
    if gold.has(case + "/ols"):
        assert same(r["ols"], gold[case + "/ols"])
    else:
        assert r["ols"] is None
    if gold.has(case + "/ols_ign"):
        assert same(ign_matrix(args[3], args[1]), gold[case + "/ols_ign"])
    if gold.has(case + "/means"):
        n = checker(*args, **kw, means=gold[case + "/means"], stds=gold[case + "/stds"])
        assert same(n["transforms"], gold[case + "/transforms_norm"])


def test_golden_edge_cases_do_what_they_claim(gold):
    args, kw = case_inputs(gold, "best_below_fg")
    r = checker(*args, **kw)
    fg = args[4]
    kept = r["best_roi"][r["best_roi"] >= 0]
    assert (r["ols_max"][kept] < fg).any(), "a kept best roi below fg"
    assert len(kept) > len(set(kept.tolist())), "two GTs share one best roi"
    args, kw = case_inputs(gold, "best0")
    r = checker(*args, **kw)
    assert r["best_roi"][-1] == 0 and r["transforms"][0, 4] >= 1, "the GT that overlaps nothing keeps roi 0"
    args, kw = case_inputs(gold, "dups")
    r = checker(*args, **kw)
    assert (r["ols"][:, 1] == r["ols"][:, 5]).all() and r["best_roi"][1] == r["best_roi"][5]


# --- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_declared_bound_exported(lib):
    from groomed_nms_amd import _lib
    header = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    for name in ("gnms_compute_targets_workspace_bytes", "gnms_compute_targets"):
        assert name + "(" in header
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.gnms_compute_targets_workspace_bytes(2, 126720, 12) == 2 * 495 * 12 * 12        # one slot per 256 rois and GT
    assert lib.gnms_compute_targets_workspace_bytes(2, 256, 12) == 2 * 12 * 12
    assert lib.gnms_compute_targets_workspace_bytes(0, 10, 12) == 0 and lib.gnms_compute_targets_workspace_bytes(2, 10, 0) == 0


def _call(lib, **over):
    """gnms_compute_targets with harmless defaults (B = 1, R = 10, M = K = 0, NULL pointers: nothing is launched on validation errors)"""
    a = dict(rois=None, rois_f64=0, B=1, R=10, ld=5, gv=None, lb=None, M=0, vc=None, gi=None, K=0, ic=None, g3=None, D3=0, r3=None, r3f=0,
             ld3=0, cen=None, cenf=0, anc=None, A=0, ac=0, tc=4, th=(0.5, 0.5, 0.0, 0.5, 0.35), mh=None, sh=None, out=(None,) * 6,
             ws=None, wsb=0)
    a.update(over)
    return lib.gnms_compute_targets(a["rois"], a["rois_f64"], a["B"], a["R"], a["ld"], a["gv"], a["lb"], a["M"], a["vc"], a["gi"], a["K"],
                                    a["ic"], a["g3"], a["D3"], a["r3"], a["r3f"], a["ld3"], a["cen"], a["cenf"], a["anc"], a["A"], a["ac"],
                                    a["tc"], *a["th"], a["mh"], a["sh"], *a["out"], a["ws"], a["wsb"], None)


def test_argument_validation_without_gpu(lib):
    fake = 1 << 20                                # never dereferenced: every call below fails before a launch
    assert _call(lib, M=257, gv=fake, lb=fake) == -2
    assert _call(lib, K=300, gi=fake, rois=fake) == -2
    assert b"at most 256" in lib.gnms_last_error()
    assert _call(lib, B=-1) == -1
    assert _call(lib, R=-5) == -1
    assert _call(lib, rois=None) == -1                                            # R > 0 and no rois
    assert _call(lib, rois=fake, ld=3) == -1                                      # fewer than 4 columns
    assert _call(lib, rois=fake, M=3, gv=None, lb=fake) == -1                     # no gts_val
    assert _call(lib, rois=fake, M=3, gv=fake, lb=None) == -1                     # no labels
    assert _call(lib, rois=fake, K=2, gi=None) == -1                              # no ignore boxes
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=6) == -1      # D3 < 7
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=25) == -1     # D3 > GNMS_TARGETS_MAX_D3
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=None, D3=16) == -1     # 3D targets of GT rows, and no gts_3d
    assert _call(lib, rois=fake, D3=-1) == -1
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=13, ac=11) == -1          # decomp reads gts_3d[:, 12:14]
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=16, ac=11, r3=fake, ld3=10) == -1   # rois_3d[:, 4:11] needs 11
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=16, ac=11) == -1          # neither rois_3d nor anchors
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=16, ac=11, anc=fake, A=6, tc=5) == -1   # tracker outside the row
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, g3=fake, D3=16, ac=3) == -1           # anchor_cols 1..3
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake) == -4                                  # no workspace
    assert _call(lib, rois=fake, M=3, gv=fake, lb=fake, ws=fake, wsb=35) == -4                # 36 bytes needed
    assert _call(lib, B=0) == 0                                                                # nothing to do


def test_python_surface_without_gpu():
    from groomed_nms_amd import overlaps, targets
    import inspect
    assert "iou_ign" in overlaps.__all__
    assert list(inspect.signature(targets.compute_targets).parameters) == [
        "gts_val", "gts_ign", "box_lbls", "rois", "fg_thresh", "ign_thresh", "bg_thresh_lo", "bg_thresh_hi", "best_thresh", "gts_3d",
        "anchors", "tracker", "rois_3d", "rois_3d_cen"]
    assert list(inspect.signature(overlaps.iou_ign).parameters) == ["box_a", "box_b", "mode", "data_type"]
    with pytest.raises(ValueError):
        overlaps.iou_ign(np.zeros((2, 4)), np.zeros((1, 4)), mode="list")
