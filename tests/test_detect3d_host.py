"""The inference post-processing (groomed_nms_amd.detect, csrc/detect3d.hip) without a GPU: a NumPy checker of the whole path, written
from the specification (the reference's operation order, lib/rpn_util.py:1087-1356) and compared with every case of
tests/golden/detect3d.npz -- the arrays the reference's own im_detect_3d returned (make_detect3d_golden.py) --, the argument checks of
the public API and the NotImplementedError branches.  test_detect3d_gpu.py reuses the checker and the comparisons for the HIP path.

Comparisons: keep lists (through the bit-exact, distinct scores), classes and trackers exactly; scores exactly; 2D boxes at the
project's decode tolerance (rtol 2e-6, atol 2e-4, tests/test_oracle_golden.py); the 3D columns at bounds derived below from fp32
rounding of their expressions (EXP_ULPS ulp for exp(), 1 ulp = 2^-23 relative per further operation), angles modulo 2 pi."""
import math

import numpy as np
import pytest
import torch

from conftest import Golden

F = np.float32
ULP = 2.0 ** -23            # fp32: relative spacing of neighbouring numbers
EXP_ULPS = 4                # exp() of the libraries involved (torch CPU, NumPy, the device's expf) is good to a few ulp

CASES = ["groomed_2d", "groomed_3d", "groomed_product", "groomed_2d_plain_alpha", "groomed_2d_acceptance", "groomed_2d_clip_scale",
         "groomed_3d_scale", "groomed_product_acceptance_scale", "groomed_2d_few_anchors", "groomed_2d_all_low", "classic_hostnms",
         "classic_clip_scale_hostnms", "classic_topn_plain_alpha_hostnms", "groomed_3d_topn"]


@pytest.fixture(scope="module")
def gold():
    return Golden("detect3d.npz")


def case_inputs(g, case):
    """(heads dict, keyword arguments of detections_from_heads) of a golden case"""
    p = case + "/"

    def conf(k, default):
        return g[p + "conf_" + k].item() if g.has(p + "conf_" + k) else default
    d = {k: g[p + k] for k in ("prob", "bbox_2d", "bbox_3d", "rois", "anchors", "bbox_means", "bbox_stds", "p2")}
    d["acceptance"] = g[p + "acceptance"] if bool(conf("use_acceptance_prob_for_nms", False)) else None
    d["scale_factor"] = float(g[p + "scale_factor"])
    d["im_hw"] = tuple(int(v) for v in g[p + "im_hw"])
    kw = dict(nms="groomed" if conf("use_nms_in_loss", False) else "classic", overlap_in_nms=str(conf("overlap_in_nms", "2d")),
              nms_thres=float(conf("nms_thres", 0.4)), nms_topN_pre=int(conf("nms_topN_pre", 3000)), groomed_topN=500,
              decomp_alpha=bool(conf("decomp_alpha", False)), clip_boxes=bool(conf("clip_boxes", False)),
              temperature=float(conf("diff_nms_temperature", 1)))
    return d, kw


def rpn_conf_of(g, case):
    """the rpn_conf the golden maker handed to the reference"""
    p = case + "/"
    c = {k: g[p + k] for k in ("anchors", "bbox_means", "bbox_stds")}
    for k in g.keys:
        if k.startswith(p + "conf_"):
            c[k[len(p) + 5:]] = g[k].item()
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------
def np_scores(prob, acceptance=None):
    """prob [A,C], acceptance [A] -> (scores fp32, cls)"""
    cls = np.argmax(prob[:, 1:], axis=1) + 1
    s = np.amax(prob[:, 1:], axis=1).astype(F)
    if acceptance is not None:
        s = s * acceptance.astype(F)
    return s, cls


def np_decode(idx, bbox_2d, bbox_3d, rois, anchors, means, stds, p2, sf, decomp_alpha):
    """The decode of the anchors `idx` of one image in fp32, the reference's operation order.  Returns dict(boxes2d, coords, raw) and the
    rounding bounds tol_coords / tol_raw [n,7] derived from the expressions."""
    m, s = np.asarray(means, np.float64).reshape(-1).astype(F), np.asarray(stds, np.float64).reshape(-1).astype(F)
    r = rois[idx].astype(F)
    d2, h = bbox_2d[idx].astype(F), bbox_3d[idx].astype(F)
    src = anchors[r[:, 4].astype(np.int64), 4:].astype(F)
    sf = F(sf)
    one, half = F(1.0), F(0.5)
    widths = r[:, 2] - r[:, 0] + one
    heights = r[:, 3] - r[:, 1] + one
    ctr_x = r[:, 0] + half * widths
    ctr_y = r[:, 1] + half * heights
    # 2D (lib/rpn_util.py:886-934, then :1190)
    dx, dy, dw, dh = [d2[:, i] * s[i] + m[i] for i in range(4)]
    pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
    pw, ph = np.exp(dw) * widths, np.exp(dh) * heights
    boxes = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw - one, pcy + half * ph - one], 1) / sf
    # 3D (:1111-1170, :1191)
    t = [h[:, i] * s[4 + i] + m[4 + i] for i in range(6)]
    mag = [np.abs(h[:, i] * s[4 + i]) + np.abs(m[4 + i]) for i in range(6)]          # magnitude of the de-normalisation's addends
    x = (t[0] * widths + ctr_x) / sf
    y = (t[1] * heights + ctr_y) / sf
    z = src[:, 0] + t[2]
    e = [np.exp(t[3 + i]) * src[:, 1 + i] for i in range(3)]
    if decomp_alpha:
        rsin = src[:, 5] + (h[:, 6] * s[11] + m[11])
        rcos = src[:, 6] + (h[:, 7] * s[12] + m[12])
        al = rcos.copy()
        pick = h[:, 8] >= half
        al[pick] = rsin[pick]
        head = h[:, 9] >= half
        al[head] = al[head] + F(math.pi)
        amag = np.where(pick, np.abs(src[:, 5]) + np.abs(h[:, 6] * s[11]) + np.abs(m[11]), np.abs(src[:, 6]) + np.abs(h[:, 7] * s[12]) + np.abs(m[12])) + math.pi
    else:
        al = (h[:, 6] * s[10] + m[10]) + src[:, 4]
        amag = np.abs(h[:, 6] * s[10]) + np.abs(m[10]) + np.abs(src[:, 4])
    coords = np.stack([x, y, z] + e + [al], 1).astype(F)
    # bounds: every fp32 operation adds at most 1 ulp of the magnitudes it combines (4 operations for x / y, 2-3 for z / alpha);
    # w h l: EXP_ULPS for exp, 1 for the product, and exp() turns the absolute error of its argument into a relative one
    tol = np.zeros(coords.shape)
    tol[:, 0] = 4 * ULP * (mag[0] * widths + np.abs(ctr_x)) / sf
    tol[:, 1] = 4 * ULP * (mag[1] * heights + np.abs(ctr_y)) / sf
    tol[:, 2] = 3 * ULP * (mag[2] + np.abs(src[:, 0]))
    for i in range(3):
        tol[:, 3 + i] = np.abs(coords[:, 3 + i]) * ULP * (EXP_ULPS + 1 + 2 * mag[3 + i])
    tol[:, 6] = 4 * ULP * amag
    # camera space (:1205-1215), float64 from the fp32 products
    Pi = np.linalg.inv(np.asarray(p2, np.float64))
    v = np.vstack(((x * z).astype(np.float64), (y * z).astype(np.float64), z.astype(np.float64), np.ones(len(z))))
    proj = Pi.dot(v)
    ry = al.astype(np.float64) + np.arctan2(-proj[2], proj[0]) + 0.5 * math.pi
    while np.any(ry > math.pi):
        ry[ry > math.pi] -= math.pi * 2
    while np.any(ry <= -math.pi):
        ry[ry <= -math.pi] += math.pi * 2
    raw = coords.copy()
    raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 6] = proj[0], proj[1], proj[2], ry
    # raw: the rounding to fp32 (1 ulp of the magnitudes summed) plus what the inputs' bounds become through p2_inv
    tol_raw = tol.copy()
    inmag = np.abs(Pi[:3, :3]).dot(np.abs(v[:3])) + np.abs(Pi[:3, 3:4])
    tv = np.vstack((tol[:, 0] * np.abs(z) + np.abs(x) * tol[:, 2] + ULP * np.abs(x * z), tol[:, 1] * np.abs(z) + np.abs(y) * tol[:, 2] + ULP * np.abs(y * z), tol[:, 2]))
    prop = np.abs(Pi[:3, :3]).dot(tv)
    for i in range(3):
        tol_raw[:, i] = 2 * ULP * inmag[i] + prop[i]
    r2 = proj[0] ** 2 + proj[2] ** 2
    tol_raw[:, 6] = tol[:, 6] + 2 * ULP * (amag + 1.5 * math.pi) + (np.abs(proj[2]) * prop[0] + np.abs(proj[0]) * prop[2]) / np.maximum(r2, 1e-300)
    return dict(boxes2d=boxes.astype(F), coords=coords, raw=raw.astype(F), tol_coords=tol, tol_raw=tol_raw)


def np_nms(scores, boxes2d, raw, nms, overlap_in_nms, nms_thres, layer_kw):
    """keep list (positions among the decoded boxes, output order) of one image, through the host oracle"""
    from oracle import oracle as O
    from groomed_nms_amd.nms._host import greedy_nms
    if nms is None:
        return np.arange(len(scores))
    if nms == "classic":
        return np.array(greedy_nms(np.hstack((boxes2d, scores[:, None])).astype(F), nms_thres, shift=1, rule="le_keep", dtype=F), np.int64)
    if len(scores) == 0:
        return np.zeros(0, np.int64)
    ov = O.iou2d(boxes2d, boxes2d)
    if overlap_in_nms != "2d":
        c = O.corners_of_cuboid_numpy_branch(raw).astype(F)
        o3 = (F(0.5) * (F(1.0) + O.iou3d_approximate(c, c, generalized=True)[1])).astype(F)
        ov = o3 if overlap_in_nms == "3d" else (ov * o3).astype(F)
    return np.asarray(O.differentiable_nms(scores, ov, nms_threshold=nms_thres, **layer_kw)["valid"], np.int64)


def np_detect(d, nms="groomed", overlap_in_nms="2d", nms_thres=0.4, nms_topN_pre=3000, groomed_topN=500, decomp_alpha=True, clip_boxes=False,
              **layer_kw):
    """the whole path for image 0 of the heads `d`: dict(rows [n,14] float64, sel, sel_scores, keep, dec)"""
    acc = d["acceptance"][0, :, 0] if d["acceptance"] is not None else None
    scores, cls = np_scores(d["prob"][0], acc)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    sel = order[:min(nms_topN_pre, len(order))]
    K = min(len(sel), groomed_topN) if nms == "groomed" else len(sel)
    dec = np_decode(sel[:K], d["bbox_2d"][0], d["bbox_3d"][0], d["rois"], d["anchors"], d["bbox_means"], d["bbox_stds"], d["p2"], d["scale_factor"],
                    decomp_alpha)
    s = scores[sel[:K]]
    keep = np_nms(s, dec["boxes2d"], dec["raw"], nms, overlap_in_nms, nms_thres, layer_kw)
    a = sel[:K][keep]
    tracker = d["rois"][a, 4].astype(np.int64)
    rows = np.hstack((dec["boxes2d"][keep], s[keep, None])).astype(F)
    rows = np.hstack((rows, cls[a, None], dec["coords"][keep], tracker[:, None]))            # float64, :1338
    if clip_boxes:
        H, W = d["im_hw"]
        rows[:, 0] = np.clip(rows[:, 0], 0, W - 1)
        rows[:, 1] = np.clip(rows[:, 1], 0, H - 1)
        rows[:, 2] = np.clip(rows[:, 2], 0, W - 1)
        rows[:, 3] = np.clip(rows[:, 3], 0, H - 1)
    return dict(rows=rows, sel=sel, sel_scores=scores[sel], keep=keep, dec=dec, scores=scores, cls=cls)


def angle_diff(a, b):
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + math.pi) % (2 * math.pi) - math.pi)


def compare_rows(got, want, chk, what=""):
    """`got` [n,14] against the reference's array `want`; `chk` = np_detect's result for the same inputs (the rounding bounds and the
    sorted scores the keep list is read from)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "%s: %r rows, the reference has %r" % (what, got.shape, want.shape)
    if len(want) == 0:
        return
    assert np.array_equal(got[:, 4], want[:, 4]), what + ": scores (and with them the keep list) differ"
    pos = {float(s): i for i, s in enumerate(chk["sel_scores"])}                             # distinct by construction
    keep_want = np.array([pos[float(s)] for s in want[:, 4]])
    assert np.array_equal(got[:, 5], want[:, 5]) and np.array_equal(got[:, 13], want[:, 13]), what + ": cls / tracker differ"
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=2e-6, atol=2e-4, err_msg=what + ": 2D boxes")
    tol = chk["dec"]["tol_coords"][keep_want]
    err = np.abs(got[:, 6:13] - want[:, 6:13])
    err[:, 6] = angle_diff(got[:, 12], want[:, 12])
    worst = np.max(err / np.maximum(tol, 1e-300), axis=0)
    print("%s: 3D columns, worst error / bound per column: %s" % (what, np.array2string(worst, precision=3)))
    assert np.all(err <= tol), "%s: 3D columns outside the fp32 rounding bound (error / bound per column %s)" % (what, worst)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_checker_matches_reference(gold, case):
    from oracle import oracle as O
    O.build()
    d, kw = case_inputs(gold, case)
    chk = np_detect(d, **kw)
    want = gold[case + "/aboxes"]
    pos = {float(s): i for i, s in enumerate(chk["sel_scores"])}
    assert [pos[float(s)] for s in want[:, 4]] == chk["keep"].tolist(), "keep list"
    compare_rows(chk["rows"], want, chk, case)
    assert int(gold[case + "/redraws"]) <= 20


def test_goldens_cover_what_they_should(gold):
    kept = {c: len(gold[c + "/aboxes"]) for c in CASES}
    assert kept["groomed_2d_all_low"] == 0 and all(v > 0 for c, v in kept.items() if c != "groomed_2d_all_low")
    assert gold["groomed_2d_few_anchors/rois"].shape[0] < 500 < gold["groomed_2d/rois"].shape[0]
    assert int(gold["groomed_3d_topn/conf_nms_topN_pre"]) < 500 < gold["groomed_3d_topn/rois"].shape[0]          # nms_topN_pre cuts below 500
    assert 500 < int(gold["classic_topn_plain_alpha_hostnms/conf_nms_topN_pre"]) < gold["classic_topn_plain_alpha_hostnms/rois"].shape[0]
    assert {float(gold[c + "/scale_factor"]) for c in CASES} >= {0.5, 0.75, 1.0, 1.5}
    d, _ = case_inputs(gold, "groomed_2d")
    assert np.any(d["bbox_3d"][0, :, 8] == 0.5) and np.any(d["bbox_3d"][0, :, 9] == 0.5), "the >= 0.5 edge of axis / head is not exercised"
    p = d["prob"][0, :, 1:]
    assert np.any(np.sum(p == p.max(1, keepdims=True), 1) > 1), "no tie between class columns"


def test_synthetic_heads_are_deterministic_and_tie_free():
    from groomed_nms_amd import synthetic
    a = synthetic.detection_heads(np.random.default_rng(3), 2, (2, 12, 12))
    b = synthetic.detection_heads(np.random.default_rng(3), 2, (2, 12, 12))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["prob"].shape == (2, 288, 4) and a["bbox_3d"].shape == (2, 288, 10) and a["rois"].shape == (288, 5)
    s = a["prob"][:, :, 1:].max(2)
    assert all(len(np.unique(s[i])) == 288 for i in range(2))
    chk = np_detect(dict(a, scale_factor=1.0, im_hw=(512, 1760)), nms=None, nms_topN_pre=288)
    bx = chk["dec"]["boxes2d"]
    assert np.all(bx[:, 2] > bx[:, 0]) and np.all(bx[:, 3] > bx[:, 1]) and bx.min() > -50 and bx[:, 2].max() < 1810
    assert synthetic.detection_heads(np.random.default_rng(3), 1, (2, 12, 12), decomp_alpha=False)["bbox_3d"].shape[2] == 7


def _heads(A=24, B=1, C=4):
    z = torch.zeros
    return dict(prob=z(B, A, C), bbox_2d=z(B, A, 4), bbox_3d=z(B, A, 10), rois=z(A, 5), anchors=np.zeros((3, 11)), bbox_means=np.zeros((1, 13)),
                bbox_stds=np.ones((1, 13)), p2=np.eye(4), scale_factor=1.0, im_hw=(10, 20))


def test_argument_checks():
    from groomed_nms_amd import detect
    from groomed_nms_amd._lib import GnmsError
    import groomed_nms_amd
    assert groomed_nms_amd.detections_from_heads is detect.detections_from_heads and groomed_nms_amd.im_detect_3d is detect.im_detect_3d
    h = _heads()
    for bad in (dict(nms="soft"), dict(overlap_in_nms="bev"), dict(nms_topN_pre=0), dict(groomed_topN=0)):
        with pytest.raises(ValueError):
            detect.detections_from_heads(**h, **bad)
    for key, val in (("prob", torch.zeros(1, 24)), ("prob", torch.zeros(1, 24, 1)), ("bbox_2d", torch.zeros(1, 24, 5)), ("bbox_2d", torch.zeros(1, 23, 4)),
                     ("bbox_3d", torch.zeros(1, 24, 9)), ("rois", torch.zeros(24, 4)), ("rois", torch.zeros(23, 5)), ("anchors", np.zeros((3, 10)))):
        with pytest.raises(ValueError):
            detect.detections_from_heads(**dict(h, **{key: val}))
    detect_plain = dict(h, bbox_3d=torch.zeros(1, 24, 7), anchors=np.zeros((3, 9)))
    if not torch.cuda.is_available():
        with pytest.raises(GnmsError):                                   # valid arguments, host tensors: no CPU fallback
            detect.detections_from_heads(**h)
        with pytest.raises(GnmsError):
            detect.detections_from_heads(**detect_plain, decomp_alpha=False)
    with pytest.raises(ValueError):
        detect.camera_constants(np.eye(3), 1.0, (10, 20), 1, torch.device("cpu"))
    with pytest.raises(ValueError):
        detect.camera_constants(np.eye(4), [1.0, 2.0, 3.0], (10, 20), 2, torch.device("cpu"))
    inv, sf, hw = detect.camera_constants(np.diag([2.0, 4.0, 1.0, 1.0]), 0.5, (10, 20), 2, torch.device("cpu"))
    assert inv.dtype == torch.float64 and inv.shape == (2, 4, 4) and inv[1, 0, 0] == 0.5 and sf.tolist() == [0.5, 0.5] and hw.tolist() == [[10, 20]] * 2


def test_library_argument_checks_without_gpu():
    import ctypes
    from groomed_nms_amd import build, _lib
    build.build()
    lib = _lib.load()
    fake = ctypes.c_void_p(256 * 1024)            # never dereferenced: every check below returns before any HIP call
    f13 = (ctypes.c_float * 13)()
    assert lib.gnms_detect3d_scores(fake, None, 1, 1, 8, 1, fake, fake, None) == -1 and b"background" in lib.gnms_last_error()
    assert lib.gnms_detect3d_scores(None, None, 1, 1, 8, 4, fake, fake, None) == -1
    assert lib.gnms_detect3d_scores(fake, fake, 0, 1, 8, 4, fake, fake, None) == -1
    assert lib.gnms_detect3d_scores(fake, None, 1, 0, 8, 4, fake, fake, None) == 0

    def dec(**k):
        a = dict(sel=fake, ld=8, K=8, A=100, b2=fake, b3=fake, D3=10, rois=fake, an=fake, n=3, cols=11, m=f13, s=f13, nc=13, dec=1, p2=fake, out2=fake,
                 c3=fake, raw=fake)
        a.update(k)
        return lib.gnms_detect3d_decode(a["sel"], a["ld"], None, 1, a["K"], a["A"], a["b2"], a["b3"], a["D3"], a["rois"], a["an"], a["n"], a["cols"],
                                        a["m"], a["s"], a["nc"], a["dec"], a["p2"], None, a["out2"], a["c3"], a["raw"], None)
    for bad in (dict(ld=4), dict(A=0), dict(D3=9), dict(cols=10), dict(nc=11), dict(p2=None), dict(m=None), dict(b2=None), dict(an=None),
                dict(out2=ctypes.c_void_p(256 * 1024 + 4)), dict(dec=0, D3=6), dict(dec=0, cols=8), dict(dec=0, nc=10)):
        assert dec(**bad) == -1, bad
    assert dec(K=0) == 0
    assert lib.gnms_detect3d_assemble(fake, 1, 4, None, fake, 8, fake, 8, fake, fake, fake, fake, 1, 8, 100, None, fake, fake, None) == -1   # ld_keep < K
    assert lib.gnms_detect3d_assemble(None, 0, 0, None, fake, 8, fake, 8, fake, fake, None, fake, 1, 8, 100, None, fake, fake, None) == -1
    assert lib.gnms_detect3d_assemble(None, 0, 0, None, fake, 8, fake, 8, fake, fake, fake, fake, 0, 8, 100, None, fake, fake, None) == 0


class _Conf(dict):
    __getattr__ = dict.__getitem__


@pytest.mark.parametrize("extra, call", [(dict(orientation_bins=8), {}), (dict(infer_2d_from_3d=True), {}), (dict(has_un=True), {}),
                                         (dict(use_el_z=True), {}), ({}, dict(synced=True)), ({}, dict(return_base=True))])
def test_excluded_branches_raise(extra, call):
    from groomed_nms_amd import detect
    conf = _Conf(anchors=np.zeros((3, 11)), bbox_means=np.zeros((1, 13)), bbox_stds=np.ones((1, 13)), nms_thres=0.4, nms_topN_pre=3000, clip_boxes=False,
                 decomp_alpha=True, **extra)

    def net(im):
        raise AssertionError("the network must not run for a branch that is not implemented")
    with pytest.raises(NotImplementedError):
        detect.im_detect_3d(np.zeros((8, 8, 3), np.float32), net, conf, lambda im: im.transpose(2, 0, 1), np.eye(4), **call)
