"""The inference post-processing on the MI355X (csrc/detect3d.hip, groomed_nms_amd.detect) against the reference's goldens and the
NumPy checker of test_detect3d_host.py, with the same comparisons; at the reference's scale (126 720 anchors) the decode is compared
field by field with the checker and the NMS stage by composition: the keep lists must be exactly what the host oracle returns for the
GPU's own decoded boxes and scores."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import Golden
from test_detect3d_host import CASES, F, angle_diff, case_inputs, compare_rows, np_decode, np_detect, np_nms, np_scores, rpn_conf_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from groomed_nms_amd import _lib, detect
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return detect


@pytest.fixture(scope="module")
def gold():
    return Golden("detect3d.npz")


def _cuda(d):
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("prob", "bbox_2d", "bbox_3d", "rois")}
    t["anchors"] = torch.from_numpy(d["anchors"]).float().cuda()
    t["acceptance_prob"] = torch.from_numpy(d["acceptance"]).cuda() if d["acceptance"] is not None else None
    return t


def _run(D, d, kw, **extra):
    t = _cuda(d)
    return D.detections_from_heads(t["prob"], t["bbox_2d"], t["bbox_3d"], t["rois"], t["anchors"], d["bbox_means"], d["bbox_stds"], d["p2"],
                                   d["scale_factor"], d["im_hw"], t["acceptance_prob"], **kw, **extra)


@pytest.mark.parametrize("case", CASES)
def test_hip_path_matches_reference(D, gold, case):
    d, kw = case_inputs(gold, case)
    det, counts = _run(D, d, kw)
    assert det.dtype == torch.float32 and det.shape[0] == 1 and det.shape[2] == 14 and counts.dtype == torch.int32
    n = int(counts[0])
    chk = np_detect(d, **kw)
    compare_rows(det[0, :n].cpu().numpy(), gold[case + "/aboxes"], chk, case)
    assert not det[0, n:].any(), "rows behind the count must be zero"


@pytest.mark.parametrize("case", CASES)
def test_drop_in_matches_reference(D, gold, case):
    d, kw = case_inputs(gold, case)
    conf = rpn_conf_of(gold, case)
    scale = d["scale_factor"]
    hs = 96
    im = np.zeros((int(round(hs / scale)), 600, 3), np.float32)
    assert im.shape[:2] == d["im_hw"]
    seen = []

    def preprocess(x):
        seen.append(x.shape)
        return np.zeros((3, hs, 8), np.float32)

    def net(x):
        assert x.is_cuda and tuple(x.shape) == (1, 3, hs, 8)
        t = _cuda(d)
        acc = t["acceptance_prob"] if t["acceptance_prob"] is not None else torch.ones(1, d["rois"].shape[0], 1).cuda()
        return None, t["prob"], t["bbox_2d"], t["bbox_3d"], None, t["rois"], acc, None
    out = D.im_detect_3d(im, net, conf, preprocess, d["p2"])
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and seen == [im.shape]
    compare_rows(out, gold[case + "/aboxes"], np_detect(d, **kw), case)


@pytest.mark.parametrize("case", ["groomed_2d", "groomed_2d_clip_scale", "groomed_3d_scale", "classic_clip_scale_hostnms"])
def test_boxes2d_bit_identical_to_bbox_transform_inv(D, gold, case):
    """the decode of the selected anchors shares its device code with gnms_bbox_transform_inv: the same bits as decoding every anchor,
    gathering, and dividing by the scale factor in fp32 (a true division, as the reference's NumPy `/=` is, lib/rpn_util.py:1190)"""
    from groomed_nms_amd import proposals
    d, kw = case_inputs(gold, case)
    _, _, mid = _run(D, d, kw, return_intermediates=True)
    t = _cuda(d)
    full = proposals.bbox_transform_inv(t["rois"], t["bbox_2d"], means=d["bbox_means"][0], stds=d["bbox_stds"][0])[0].cpu().numpy()
    K = mid["boxes2d"].shape[1]
    idx = mid["sel_index"][0, :K].cpu().numpy()
    want = full[idx] / F(d["scale_factor"])
    assert want.dtype == np.float32 and np.array_equal(mid["boxes2d"][0].cpu().numpy(), want)


@functools.lru_cache(maxsize=None)
def _scene(B_objects=(12, 7), grid=(32, 110, 36), seed=7):
    """the at-scale heads (126 720 anchors, two images that keep different numbers of boxes): built once, shared, never written to"""
    from groomed_nms_amd import synthetic
    parts = [synthetic.detection_heads(np.random.default_rng(seed), 1, grid, n_objects=n) for n in B_objects]
    d = dict(parts[0])
    for k in ("rois", "anchors", "bbox_means", "bbox_stds"):
        assert all(np.array_equal(p[k], d[k]) for p in parts)
    for k in ("prob", "bbox_2d", "bbox_3d", "acceptance"):
        d[k] = np.concatenate([p[k] for p in parts])
    d["scale_factor"], d["im_hw"] = 0.75, (683, 2347)
    return d


def raw_from_own_coords(c3, p2):
    """coords_3d_raw recomputed in float64 from the GPU's OWN coords_3d [n,7] (fp32): the fp32 products x z and y z, p2_inv applied in
    float64 term by term, rotation_y = alpha + atan2(-z3, x3) + pi/2 wrapped into (-pi, pi], everything rounded to fp32 at the end.
    No exp() is involved, so nothing but the float64 evaluation itself separates this from the kernel.  Returns (raw fp32 [n,7], bound
    [n,7]).  Bounds: x3 y3 z3 are four float64 products and three sums, in any order wrong by at most 8 * 2^-53 of the summed magnitudes,
    and two roundings to fp32 of values that close differ by at most one fp32 spacing; rotation_y adds atan2 (a few float64 ulp in any
    libm) and the wrap, all on values below 4 pi: 2^-48 covers it, again plus one fp32 spacing.  w h l are copies: exact."""
    c3 = np.asarray(c3, F)
    Pi = np.linalg.inv(np.asarray(p2, np.float64))
    X, Y, Z = (c3[:, 0] * c3[:, 2]).astype(np.float64), (c3[:, 1] * c3[:, 2]).astype(np.float64), c3[:, 2].astype(np.float64)
    proj = [Pi[i, 0] * X + Pi[i, 1] * Y + Pi[i, 2] * Z + Pi[i, 3] for i in range(3)]
    mag = [np.abs(Pi[i, 0] * X) + np.abs(Pi[i, 1] * Y) + np.abs(Pi[i, 2] * Z) + abs(Pi[i, 3]) for i in range(3)]
    ry = c3[:, 6].astype(np.float64) + np.arctan2(-proj[2], proj[0]) + 0.5 * math.pi
    while np.any(ry > math.pi):
        ry[ry > math.pi] -= math.pi * 2
    while np.any(ry <= -math.pi):
        ry[ry <= -math.pi] += math.pi * 2
    raw = c3.copy()
    tol = np.zeros(c3.shape)
    for i in range(3):
        raw[:, i] = proj[i]
        tol[:, i] = np.spacing(np.abs(raw[:, i])) + 2.0 ** -50 * mag[i]
    raw[:, 6] = ry
    tol[:, 6] = np.spacing(np.maximum(np.abs(raw[:, 6]), F(1.0))) + 2.0 ** -48
    return raw, tol


def check_raw_against_own_coords(g3, graw, p2, what):
    want, tol = raw_from_own_coords(g3, p2)
    err = np.abs(graw.astype(np.float64) - want.astype(np.float64))
    err[:, 6] = angle_diff(graw[:, 6], want[:, 6])
    same = np.mean(graw[:, [0, 1, 2, 6]] == want[:, [0, 1, 2, 6]], axis=0)
    print("%s: coords_3d_raw against float64 from the GPU's own coords_3d: worst error / bound per column %s, identical bits x3 y3 z3 ry %s"
          % (what, np.array2string(np.max(err / np.maximum(tol, 1e-300), axis=0), precision=3), np.array2string(same, precision=4)))
    assert np.array_equal(graw[:, 3:6], g3[:, 3:6]), what + ": w h l of coords_3d_raw are copies of coords_3d"
    assert np.all(err <= tol), "%s: coords_3d_raw is not the float64 back-projection of coords_3d (rows %s)" % (what, np.nonzero(np.any(err > tol, 1))[0][:8])


def test_raw_is_the_float64_back_projection_of_own_coords(D, gold):
    """p2_inv must be applied in float64 (lib/rpn_util.py:1205-1215 is NumPy): coords_3d_raw against a float64 recomputation from the
    kernel's own coords_3d, to one fp32 spacing -- the propagated bounds of np_decode are far wider than what fp32 arithmetic here
    would change.  All 3000 selected anchors of both at-scale images, and a golden case with decomp_alpha off."""
    d = _scene()
    _, _, mid = _run(D, d, dict(nms=None, nms_topN_pre=3000), return_intermediates=True)
    assert mid["coords_3d_raw"].shape == (2, 3000, 7)
    for b in range(2):
        check_raw_against_own_coords(mid["coords_3d"][b].cpu().numpy(), mid["coords_3d_raw"][b].cpu().numpy(), d["p2"], "image %d" % b)
    d, kw = case_inputs(gold, "groomed_2d_plain_alpha")
    _, _, mid = _run(D, d, kw, return_intermediates=True)
    check_raw_against_own_coords(mid["coords_3d"][0].cpu().numpy(), mid["coords_3d_raw"][0].cpu().numpy(), d["p2"], "groomed_2d_plain_alpha")


@pytest.mark.parametrize("nms, overlap", [("groomed", "2d"), ("classic", "2d")])
def test_at_scale_decode_fieldwise_and_nms_by_composition(D, nms, overlap):
    d = _scene()
    A = d["rois"].shape[0]
    assert A == 126720
    kw = dict(nms=nms, overlap_in_nms=overlap, nms_topN_pre=3000, groomed_topN=500, clip_boxes=True)
    det, counts, mid = _run(D, d, kw, return_intermediates=True)
    counts = counts.cpu().numpy()
    K = mid["boxes2d"].shape[1]
    assert K == (500 if nms == "groomed" else 3000)
    for b in range(2):
        s, cls = np_scores(d["prob"][b], d["acceptance"][b, :, 0])
        assert np.array_equal(mid["scores"][b].cpu().numpy(), s) and np.array_equal(mid["cls_pred"][b].cpu().numpy(), cls)
        sel = np.argsort(-s.astype(np.float64), kind="stable")[:3000]
        assert np.array_equal(mid["sel_index"][b].cpu().numpy(), sel)
        chk = np_decode(sel[:K], d["bbox_2d"][b], d["bbox_3d"][b], d["rois"], d["anchors"], d["bbox_means"], d["bbox_stds"], d["p2"], d["scale_factor"], True)
        g2, g3, graw = [mid[k][b].cpu().numpy() for k in ("boxes2d", "coords_3d", "coords_3d_raw")]
        np.testing.assert_allclose(g2, chk["boxes2d"], rtol=2e-6, atol=2e-4)
        for got, want, tol, what in ((g3, chk["coords"], chk["tol_coords"], "coords_3d"), (graw, chk["raw"], chk["tol_raw"], "coords_3d_raw")):
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            err[:, 6] = angle_diff(got[:, 6], want[:, 6])
            worst = np.max(err / np.maximum(tol, 1e-300), axis=0)
            print("image %d %s: worst error / bound per column %s" % (b, what, np.array2string(worst, precision=3)))
            assert np.all(err <= tol), (what, worst)
        # the NMS by composition: the host oracle on the GPU's own boxes and scores
        gs = mid["sel_scores"][b, :K].cpu().numpy()
        keep = np_nms(gs, g2, graw, nms, overlap, 0.4, {})
        n = int(counts[b])
        assert mid["keep"][b, :n].cpu().numpy().tolist() == keep.tolist()
        rows = det[b, :n].cpu().numpy()
        a = sel[:K][keep]
        H, W = d["im_hw"]
        want2 = g2[keep].copy()
        want2[:, 0::2] = np.clip(want2[:, 0::2], 0, W - 1)
        want2[:, 1::2] = np.clip(want2[:, 1::2], 0, H - 1)
        assert np.array_equal(rows[:, :4], want2) and np.array_equal(rows[:, 4], gs[keep]) and np.array_equal(rows[:, 5], cls[a])
        assert np.array_equal(rows[:, 6:13], g3[keep]) and np.array_equal(rows[:, 13], d["rois"][a, 4])
        assert not det[b, n:].any()
    assert counts[0] != counts[1], "the two images were built to keep different numbers of boxes"


def test_zero_kept_and_fewer_anchors_than_topn(D, gold):
    d, kw = case_inputs(gold, "groomed_2d_all_low")
    det, counts = _run(D, d, kw)
    assert int(counts[0]) == 0 and det.shape == (1, 500, 14) and not det.any()
    d, kw = case_inputs(gold, "groomed_2d_few_anchors")
    det, counts = _run(D, d, kw)
    assert det.shape == (1, d["rois"].shape[0], 14) and 0 < int(counts[0]) == len(gold["groomed_2d_few_anchors/aboxes"])
    det, counts = _run(D, d, dict(kw, nms=None))
    assert int(counts[0]) == d["rois"].shape[0] and np.all(np.diff(det[0, :, 4].cpu().numpy()) < 0)


def _device_call(D, d, kw):
    """every argument on the device already: the call is stream-ordered launches only"""
    t = _cuda(d)
    inv, sf, hw = D.camera_constants(d["p2"], d["scale_factor"], d["im_hw"], 1)

    def call():
        return D.detections_from_heads(t["prob"], t["bbox_2d"], t["bbox_3d"], t["rois"], t["anchors"], d["bbox_means"], d["bbox_stds"], None, sf, hw,
                                       t["acceptance_prob"], p2_inv=inv, **kw)
    return call


@pytest.mark.parametrize("case", ["groomed_2d_clip_scale", "groomed_product_acceptance_scale", "classic_clip_scale_hostnms"])
def test_graph_replay_equals_eager(D, gold, case):
    """Captured: the WHOLE of detections_from_heads (scores, top-K, decode, overlaps + layer or greedy NMS, assembly) -- with device
    tensors in there is no host read anywhere in it.  (Up to GNMS_MAX_BOXES anchors; above that the top-K takes a stream-ordered
    temporary, which this test does not capture.)"""
    d, kw = case_inputs(gold, case)
    call = _device_call(D, d, kw)
    det0, cnt0 = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        det, cnt = call()
    for _ in range(3):
        det.zero_()
        cnt.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(det, det0) and torch.equal(cnt, cnt0)
    assert int(cnt0[0]) == len(gold[case + "/aboxes"])


def test_graph_replay_equals_eager_at_scale(D):
    """126 720 anchors, B = 2, 3000 -> 500: under capture gnms_select_topk takes its radix pre-selection with the stream-ordered
    temporary (the cooperative launch is for eager calls only); the replay must give what the eager call gave"""
    d = _scene()
    t = _cuda(d)
    inv, sf, hw = D.camera_constants(d["p2"], d["scale_factor"], d["im_hw"], 2)

    def call():
        return D.detections_from_heads(t["prob"], t["bbox_2d"], t["bbox_3d"], t["rois"], t["anchors"], d["bbox_means"], d["bbox_stds"], None, sf, hw,
                                       t["acceptance_prob"], p2_inv=inv, clip_boxes=True)
    det0, cnt0 = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        det, cnt = call()
    for _ in range(2):
        det.zero_()
        cnt.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(det, det0) and torch.equal(cnt, cnt0)
    assert cnt0[0] != cnt0[1] and int(cnt0.min()) > 0


def test_two_streams_at_once_equal_eager(D, gold):
    cases = ["groomed_3d_scale", "classic_hostnms"]
    calls = [_device_call(D, *case_inputs(gold, c)) for c in cases]
    want = [c() for c in calls]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in cases]
    got = [None, None]
    for rep in range(5):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                got[i] = calls[i]()
    for st in streams:
        st.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g[0], w[0]) and torch.equal(g[1], w[1])
