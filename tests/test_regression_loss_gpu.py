"""GPU tests of the box regression, 2D IoU and uncertainty terms of the RPN loss (groomed_nms_amd/regression.py, csrc/regression.hip)
against the reference's goldens (tests/golden/regression.npz) and the float64 restatement of tests/test_regression_loss_host.py.

The rule: |gpu - restatement| <= max(4 e_ref, 4 float32 ulps of the largest entry), e_ref = |reference - restatement|
of the same quantity in the same golden case; the synthetic shapes have no reference and take 4 float32 ulps.  The active set, the finite
counts and the weighting decision are exact.  Measured per golden case: DESIGN.md 3.15 (each test prints its figures before it asserts)."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_regression_loss_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = ("bbox_2d", "bbox_3d", "acceptance")
ARRAYS = ("transforms", "raw_gt", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor")
FakeSample = collections.namedtuple("FakeSample", ["fg_index", "fg_counts", "counts"])


@pytest.fixture(scope="module")
def dev():
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def kwargs_of(kw):
    return dict(means=kw["means"], stds=kw["stds"], bbox_2d_lambda=kw["bbox_2d_lambda"], bbox_3d_lambda=kw["bbox_3d_lambda"],
                bbox_axis_head_lambda=kw["bbox_axis_head_lambda"], iou_2d_lambda=kw["iou_2d_lambda"],
                use_acceptance_prob_in_regression_loss=kw["use_acceptance"], bbox_un_lambda=kw["bbox_un_lambda"],
                bbox_un_dynamic=kw["bbox_un_dynamic"])


def sample_of(fg_lists, fg_num, R, dev):
    """a Sample's three fields that regression_loss reads, from per-image active lists"""
    B = len(fg_lists)
    idx = np.full((B, R), -1, np.int32)
    counts = np.zeros((B, 6), np.int32)
    for b, l in enumerate(fg_lists):
        idx[b, :len(l)] = l
        counts[b, 2], counts[b, 4] = fg_num[b], len(l)
    return FakeSample(_t(idx, dev), _t(counts[:, 4].copy(), dev), _t(counts, dev))


def run_gpu(dev, d, sample, kw, state=None, upstream=None, views=None):
    """the call and the backward; everything back on the host as NumPy.  d: the arrays; views: optional device tensors to pass instead"""
    from groomed_nms_amd import regression
    t = {k: _t(d[k], dev) for k in ARRAYS}
    t.update(views or {})
    heads = {k: (_t(d[k], dev).requires_grad_(True) if d.get(k) is not None else None) for k in HEADS}
    loss, stats = regression.regression_loss(heads["bbox_2d"], heads["bbox_3d"], heads["acceptance"], (t["transforms"], t["raw_gt"]), sample,
                                             t["rois"], t["rois_3d"], t["rois_3d_cen"], t["p2"], t["scale_factor"], un_state=state, **kwargs_of(kw))
    (loss if upstream is None else loss * upstream).backward()
    torch.cuda.synchronize()
    out = {"loss": float(loss.detach().cpu()), "counts": stats["counts"].cpu().numpy()}
    out["stats"] = {k: float(stats[k].cpu()) for k in H.STAT_NAMES + ["bbox_un_lambda"]}
    for k in HEADS:
        out["grad_" + k] = heads[k].grad.cpu().numpy() if heads[k] is not None else None
    return out


def check(g, r, e, what):
    """exact: the counts and decisions; by the rule: loss, statistics, gradients.  e: e_ref per quantity, or None (synthetic)"""
    c = g["counts"]
    assert c[0] == r["n"], what
    ratios = {}
    if r["n"] == 0:
        assert g["loss"] == 0.0 and all(np.isnan(g["stats"][k]) for k in H.STAT_NAMES)
    else:
        assert list(c[1:10]) == r["finite_unweighted"], (what, c)
        if "finite_weighted" in r:
            assert list(c[10:17]) == r["finite_weighted"], (what, c)
        assert tuple(c[17:20]) == r["finite_iou"], (what, c)
        assert bool(c[20]) == r["weighted"] and bool(c[21]) == r["has_iou"], what
        for k in ["loss"] + H.STAT_NAMES + ["bbox_un_lambda"]:
            want = r["loss"] if k == "loss" else r["stats"][k]
            got = g["loss"] if k == "loss" else g["stats"][k]
            if np.isnan(want):
                assert np.isnan(got), (what, k, got)
                continue
            tol = max(4 * (e.get("weight" if k == "bbox_un_lambda" else k, 0.0) if e else 0.0), 4 * ulp32(want))
            ratios[k] = abs(got - want) / tol if tol else 0.0
            assert abs(got - want) <= tol, (what, k, got, want, tol)
    mask = np.zeros(r["grad_bbox_2d"].shape[:2], bool)
    mask[r["active"]] = True
    for k in HEADS:
        got, want = g["grad_" + k], r["grad_" + k]
        if got is None:
            continue
        assert not got[~mask].any(), "%s: %s is not 0 off the active set" % (what, k)
        top = float(np.abs(want).max())
        tol = max(4 * (e.get("grad_" + k, 0.0) if e else 0.0), 4 * ulp32(top))
        d = float(np.abs(got.astype(np.float64) - want).max())
        ratios["grad_" + k] = d / tol if tol else 0.0
        assert d <= tol, (what, k, d, tol)
    print("%s: |gpu - restatement| / tolerance: %s" % (what, " ".join("%s %.3f" % (k, v) for k, v in ratios.items())))
    return ratios


def golden_sample(cid, dev):
    """the real sampler on the case's label column, read in place from the transforms rows"""
    from groomed_nms_amd import sampling
    c = H.case_of(cid)
    tr = _t(c["transforms"], dev)
    s = sampling.sample_anchors(tr[..., 4], _t(c["prob"], dev), _t(c["val_counts"], dev), box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])
    return s, tr


@pytest.mark.parametrize("cid", H.case_ids())
def test_golden_cases(dev, cid):
    c, r, e = H.case_of(cid), H.restated(cid), H.reference_errors(cid)
    s, tr = golden_sample(cid, dev)
    want = H.sampled(cid)
    fg_counts = s.fg_counts.cpu().numpy()
    for b, l in enumerate(want["fg_lists"]):                       # the active set
        assert fg_counts[b] == len(l) and np.array_equal(s.fg_index[b, :len(l)].cpu().numpy(), l)
    assert np.array_equal(s.counts.cpu().numpy(), want["counts"])
    state = _t(np.asarray(c["state_in"], np.float64), dev) if c["kw"]["bbox_un_dynamic"] else None
    g = run_gpu(dev, c, s, c["kw"], state=state, views={"transforms": tr})
    check(g, r, e, cid)
    if state is not None:
        got = state.cpu().numpy()
        assert got[0] == r["state_out"][0] == c["state_out"][0]
        tol = max(4 * e["weight"], 4 * ulp32(r["state_out"][1]))
        print("%s: weight %.9g, restatement %.9g, reference %.9g, tolerance %.3g" % (cid, got[1], r["state_out"][1], c["state_out"][1], tol))
        assert abs(got[1] - r["state_out"][1]) <= tol and abs(got[1] - float(c["state_out"][1])) <= tol
        assert got[1] == g["stats"]["bbox_un_lambda"]


def test_three_dynamic_steps_through_one_state(dev):
    """Only the chaining: the state that step k leaves is the input of step k + 1, checked by the rule against the restatement fed with
    this run's own incoming state (the recorded weight of each step is checked from the recorded state in test_golden_cases); a step
    without an active anchor leaves the state's bits"""
    for shape in ("r210", "r1332"):
        state = _t(np.zeros(2), dev)
        for k in range(3):
            cid = "%s/dyn3_s%d" % (shape, k)
            c, e, sm = H.case_of(cid), H.reference_errors(cid), H.sampled(cid)
            came_in = tuple(state.cpu().numpy().tolist())
            r = H.restate(*[c[x] for x in HEADS + ARRAYS], sm["fg_lists"], sm["counts"][:, 2], state_in=came_in, **c["kw"])
            s, tr = golden_sample(cid, dev)
            g = run_gpu(dev, c, s, c["kw"], state=state, views={"transforms": tr})
            check(g, r, e, cid + " (chained)")
            got = state.cpu().numpy()
            tol = max(4 * e["weight"], 4 * ulp32(r["state_out"][1]))
            print("%s: n_frames %g weight %.9g (restatement %.9g, reference %.9g, tolerance %.3g)" % (cid, got[0], got[1], r["state_out"][1],
                                                                                                   c["state_out"][1], tol))
            assert got[0] == k + 1 == r["state_out"][0] and abs(got[1] - r["state_out"][1]) <= tol
        before = state.cpu().numpy().view(np.int64).copy()
        empty = sample_of([[], []], [0, 0], c["bbox_2d"].shape[1], dev)
        g = run_gpu(dev, c, empty, c["kw"], state=state)
        assert g["loss"] == 0.0 and np.array_equal(state.cpu().numpy().view(np.int64), before)
        assert not g["grad_bbox_2d"].any() and not g["grad_bbox_3d"].any() and not g["grad_acceptance"].any()
        assert all(np.isnan(g["stats"][k]) for k in H.STAT_NAMES) and g["stats"]["bbox_un_lambda"] == state.cpu().numpy()[1]


# ---------------------------------------------------------------------------------------------- synthetic shapes

REF_KW = dict(bbox_2d_lambda=1.0, bbox_3d_lambda=1.0, bbox_axis_head_lambda=0.35, iou_2d_lambda=1.0, use_acceptance=True, bbox_un_lambda=0.0,
              bbox_un_dynamic=True)


def synth(R, actives, fg_num=None, seed=0, D3=11, p2_rows=3):
    """random heads near their targets (every sampled box overlaps its target) for B = len(actives) images with the given active counts"""
    rng = np.random.default_rng(1000 + seed)
    B = len(actives)
    f = np.float32
    xy = rng.uniform(0, 500, (B, R, 2))
    wh = rng.uniform(16, 90, (B, R, 2))
    d = dict(rois=np.concatenate([xy, xy + wh, rng.integers(0, 9, (B, R, 1))], 2).astype(f))
    d["rois_3d"] = np.concatenate([d["rois"][:, :, :4], rng.uniform(5, 40, (B, R, 1)), rng.uniform(0.5, 4, (B, R, 3)), rng.uniform(-3, 3, (B, R, 3))], 2).astype(f)
    d["rois_3d_cen"] = (xy + wh / 2 + rng.normal(0, 2, (B, R, 2))).astype(f)
    d["bbox_2d"] = rng.normal(0, 0.1, (B, R, 4)).astype(f)
    d["bbox_3d"] = rng.normal(0, 0.8, (B, R, D3)).astype(f)               # some differences beyond 1: both branches of smooth-L1
    d["bbox_3d"][:, :, 8:10] = rng.uniform(0.02, 0.98, (B, R, 2))
    d["acceptance"] = rng.uniform(0.05, 1.0, (B, R)).astype(f)
    d["transforms"] = rng.normal(0, 0.3, (B, R, 14)).astype(f)
    d["transforms"][:, :, :4] = rng.normal(0, 0.1, (B, R, 4))
    d["raw_gt"] = rng.uniform(-3, 3, (B, R, 21)).astype(f)
    d["raw_gt"][:, :, 12:15] = rng.uniform(-20, 60, (B, R, 3))
    d["raw_gt"][:, :, 19:21] = rng.integers(0, 2, (B, R, 2))
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])[:p2_rows]
    d["p2"] = np.stack([p2 * (1 + 0.01 * b) for b in range(B)])
    d["scale_factor"] = rng.uniform(0.7, 1.3, B)
    d["fg_lists"] = [np.sort(rng.choice(R, k, replace=False)) for k in actives]
    d["fg_num"] = list(actives) if fg_num is None else list(fg_num)
    d["kw"] = dict(REF_KW, means=np.round(rng.normal(0, 0.1, 13), 3), stds=np.round(rng.uniform(0.5, 1.5, 13), 3))
    return d


def restate_synth(d, state_in=(0.0, 0.0), **over):
    return H.restate(*[d[k] for k in HEADS + ARRAYS], d["fg_lists"], d["fg_num"], state_in=state_in, **dict(d["kw"], **over))


@pytest.mark.parametrize("actives", [(0, 0), (1, 0), (0, 1), (63, 64), (65, 256), (257, 1), (300, 300)])
def test_reduction_sizes(dev, actives):
    """active anchors per image around the wave (64) and the workgroup (256); R = 300: two workgroups per image"""
    d = synth(300, actives, seed=sum(actives))
    state = _t(np.array([3.0, 1.25]), dev)
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=state)
    r = restate_synth(d, state_in=(3.0, 1.25))
    check(g, r, None, "actives %s" % (actives,))
    got = state.cpu().numpy()
    assert got[0] == r["state_out"][0] and abs(got[1] - r["state_out"][1]) <= 4 * ulp32(r["state_out"][1])


def test_all_foreground_spans_eight_workgroups(dev):
    d = synth(2048, (2048, 2048), seed=7, D3=10, p2_rows=4)
    state = _t(np.zeros(2), dev)
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 2048, dev), d["kw"], state=state)
    check(g, restate_synth(d), None, "R = 2048, all foreground")


def test_image_without_quota_beside_one_with(dev):
    """counts[b][2] == 0 (:617): the image's anchors are active and their IoUs are 0"""
    d = synth(300, (40, 70), fg_num=(0, 70), seed=3)
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=_t(np.zeros(2), dev))
    r = restate_synth(d)
    assert r["finite_iou"] == (110, 70, 70)
    check(g, r, None, "fg_num (0, 70)")
    d["kw"]["bbox_2d_lambda"] = 0.0
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=_t(np.zeros(2), dev))
    check(g, restate_synth(d), None, "fg_num (0, 70), no 2D term")
    assert not g["grad_bbox_2d"][0].any() and g["grad_bbox_2d"][1].any()


def test_without_the_3d_term(dev):
    """bbox_3d_lambda == 0 (:1211): no 3D term, no axis / head / conf statistics, the running weight is not updated"""
    d = synth(300, (40, 70), seed=17)
    d["kw"].update(bbox_3d_lambda=0.0)
    state = _t(np.array([4.0, 0.75]), dev)
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=state)
    r = restate_synth(d, state_in=(4.0, 0.75))
    assert r["stats"]["un"] > 0 and all(np.isnan(r["stats"][k]) for k in ("axis", "head", "conf")) and not r["weighted"]
    check(g, r, None, "bbox_3d_lambda 0")
    assert state.cpu().numpy().tolist() == [4.0, 0.75] and not g["grad_bbox_3d"].any()


def test_missed_target_and_nan_entry(dev):
    """a sampled box that misses its target: IoU 0, -log IoU = inf is dropped, its gradient is 0 and the loss stays finite.  A NaN in
    one bbox_3d entry: that term's finite count drops by one, the other terms and every gradient stay finite"""
    d = synth(300, (70, 65), seed=5)
    d["kw"]["bbox_2d_lambda"] = 0.0
    base = restate_synth(d)
    miss, nan = d["fg_lists"][0][3], d["fg_lists"][1][64]
    d["bbox_2d"][0, miss, 0] = 40.0
    d["bbox_3d"][1, nan, 1] = np.nan
    g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=_t(np.zeros(2), dev))
    r = restate_synth(d)
    assert r["finite_iou"] == (135, 134, 134) and r["finite_unweighted"] == [135, 134] + [135] * 7 and r["finite_weighted"][1] == 134
    for k in HEADS:
        assert np.isfinite(g["grad_" + k]).all(), k
    assert np.isfinite(g["loss"]) and not g["grad_bbox_2d"][0, miss].any() and g["grad_bbox_3d"][1, nan, 1] == 0.0
    for k in ("cen", "bbox_3d", "total"):          # the NaN reaches the statistic that decodes it, and no term
        assert np.isnan(g["stats"][k]) == (k == "cen")
    check(g, r, None, "missed target, NaN entry")
    assert list(g["counts"][1:10]) != base["finite_unweighted"]


def test_strided_rows_and_side_stream(dev):
    """transforms, raw_gt, rois and rois_3d read in place from wider rows; 12 bbox_3d columns; an upstream gradient; a side stream"""
    from groomed_nms_amd import regression
    d = synth(300, (65, 130), seed=11, D3=12)
    r = restate_synth(d)
    wide = {}
    for k, cols in (("transforms", 23), ("raw_gt", 24), ("rois", 7), ("rois_3d", 13)):
        w = torch.full((2, 300, cols), 9.0, device=dev)
        w[:, :, :d[k].shape[2]] = _t(d[k], dev)
        wide[k] = w[:, :, :d[k].shape[2]]
        assert not wide[k].is_contiguous()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        g = run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 300, dev), d["kw"], state=_t(np.zeros(2), dev), upstream=0.5, views=wide)
    for k in HEADS:
        g["grad_" + k] = g["grad_" + k] * 2.0                      # (exact)
    check(g, r, None, "strided rows")
    assert not g["grad_bbox_3d"][:, :, 10:].any()
    assert regression.N_STATS == len(regression.STAT_NAMES)


def test_two_calls_give_the_same_bits(dev):
    d = synth(2048, (1500, 700), seed=13)
    runs = [run_gpu(dev, d, sample_of(d["fg_lists"], d["fg_num"], 2048, dev), d["kw"], state=_t(np.array([7.0, 2.0]), dev)) for _ in range(2)]
    a, b = runs
    assert np.float32(a["loss"]).tobytes() == np.float32(b["loss"]).tobytes()
    for k in a["stats"]:
        assert np.float64(a["stats"][k]).tobytes() == np.float64(b["stats"][k]).tobytes(), k
    for k in HEADS:
        assert np.array_equal(a["grad_" + k].view(np.int32), b["grad_" + k].view(np.int32)), k


def test_graph_capture_with_sampler_and_classification(dev):
    """sample_anchors, classification_loss and regression_loss in one graph on a side stream: each of three replays returns the bits of
    the eager call of the same step, and un_state advances once per replay"""
    from groomed_nms_amd import sampling, regression
    c = H.case_of("r1332/both_cut")
    rng = np.random.default_rng(5)
    cls = _t(rng.normal(0, 1.5, c["prob"].shape).astype(np.float32), dev).requires_grad_(True)
    heads = [_t(c[k], dev).requires_grad_(True) for k in HEADS]
    t = {k: _t(c[k], dev) for k in ARRAYS + ("prob", "val_counts")}
    kw = kwargs_of(c["kw"])

    def step(state):
        s = sampling.sample_anchors(t["transforms"][..., 4], t["prob"], t["val_counts"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])
        lc, _ = sampling.classification_loss(cls, s, fg_fraction=c["fg_fraction"])
        lr, st = regression.regression_loss(*heads, (t["transforms"], t["raw_gt"]), s, t["rois"], t["rois_3d"], t["rois_3d_cen"], t["p2"],
                                            t["scale_factor"], un_state=state, **kw)
        grads = torch.autograd.grad(lc + lr, [cls] + heads)
        return [lc.detach(), lr.detach(), st["total"], st["bbox_un_lambda"], st["cen"]] + list(grads)

    eager_state = _t(np.zeros(2), dev)
    eager = []
    for _ in range(3):
        eager.append([x.cpu().numpy().copy() for x in step(eager_state)] + [eager_state.cpu().numpy().copy()])
    state = _t(np.zeros(2), dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = step(state)
    torch.cuda.synchronize()
    assert state.cpu().numpy().tolist() == [0.0, 0.0]              # capturing runs nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in outs] + [state.cpu().numpy()]
        assert got[-1][0] == k + 1
        for i, (a, b) in enumerate(zip(got, eager[k])):
            assert a.tobytes() == b.tobytes(), "replay %d, output %d" % (k, i)


def test_argument_errors_return_their_codes(dev):
    from groomed_nms_amd import regression
    d = synth(64, (3, 4))
    s = sample_of(d["fg_lists"], d["fg_num"], 64, dev)
    t = {k: _t(d[k], dev) for k in HEADS + ARRAYS}
    args = [t[k] for k in HEADS] + [(t["transforms"], t["raw_gt"]), s] + [t[k] for k in ARRAYS[2:]]
    with pytest.raises(ValueError, match="p2"):
        regression.regression_loss(*args[:8], t["p2"][:, :2], t["scale_factor"], **kwargs_of(dict(d["kw"], bbox_un_dynamic=False)))
    with pytest.raises(ValueError, match="un_state"):
        regression.regression_loss(*args, un_state=torch.zeros(2, device=dev), **kwargs_of(d["kw"]))
    loss, stats = regression.regression_loss(*args, un_state=regression.new_un_state(dev), **kwargs_of(d["kw"]))
    assert np.isfinite(float(loss.cpu())) and int(stats["counts"][0].cpu()) == 7
