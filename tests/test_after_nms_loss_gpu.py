"""GPU tests of the after-NMS block of the RPN loss (groomed_nms_amd/after_nms.py, csrc/after_nms.hip, gnms_aploss_tail) against the
reference's goldens (tests/golden/after_nms.npz) and the restatement of tests/test_after_nms_loss_host.py.

The rule: |gpu - restatement| <= max(4 e_ref, 4 float32 ulps of the largest entry), e_ref = |reference - restatement|
of the same quantity in the same golden case; the synthetic shapes have no reference and take 4 float32 ulps.  Selection index sets,
targets, counts and img_cnt are exact, gradients exactly 0 off the selection.  Measured per golden case: DESIGN.md 3.16 (each test
prints its figures before it asserts)."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_after_nms_loss_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ("bbox_2d", "bbox_3d", "raw_gt", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor", "gts_val", "gts_3d", "val_counts")
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


def sample_of(fg_lists, fg_num, R, dev):
    """a Sample's three fields that after_nms_loss reads, from per-image foreground lists"""
    B = len(fg_lists)
    idx = np.full((B, R), -1, np.int32)
    counts = np.zeros((B, 6), np.int32)
    for b, l in enumerate(fg_lists):
        idx[b, :len(l)] = l
        counts[b, 2], counts[b, 4] = fg_num[b], len(l)
    return FakeSample(_t(idx, dev), _t(counts[:, 4].copy(), dev), _t(counts, dev))


def call(dev, d, sample, kw, views=None):
    """-> (loss, info, heads): the call on device copies of the arrays `d`; views: device tensors to pass instead"""
    from groomed_nms_amd import after_nms
    t = {k: _t(d[k], dev) for k in ARRAYS}
    t.update(views or {})
    heads = {k: (_t(d[k], dev).requires_grad_(True) if d.get(k) is not None else None) for k in ("prob", "acceptance")}
    loss, info = after_nms.after_nms_loss(heads["prob"], heads["acceptance"], t["bbox_2d"], t["bbox_3d"], (None, t["raw_gt"]), sample, t["rois"],
                                          t["rois_3d"], t["rois_3d_cen"], t["p2"], t["scale_factor"], t["gts_val"], t["gts_3d"], t["val_counts"],
                                          means=d["means"], stds=d["stds"], **H.api_kw(kw))
    return loss, info, heads


def run_gpu(dev, d, sample, kw, upstream=None, views=None):
    """the call and the backward; everything back on the host as NumPy"""
    loss, info, heads = call(dev, d, sample, kw, views)
    if loss.requires_grad:
        (loss if upstream is None else loss * upstream).backward()
    torch.cuda.synchronize()
    out = {"loss": float(loss.detach().cpu())}
    for k, v in info.items():
        out[k] = v.cpu().numpy()
    for k in ("prob", "acceptance"):
        out["grad_" + k] = heads[k].grad.cpu().numpy() if (heads[k] is not None and heads[k].grad is not None) else None
    return out


def check(g, r, e, what, kw):
    """exact: counts, index sets, targets, img_cnt, zeros off the selection; by the rule: loss, statistic, gradients.
    e: e_ref per quantity, or None (synthetic)"""
    B = len(r["sel"])
    assert int(g["img_cnt"]) == r["img_cnt"], what
    for b in range(B):
        n = len(r["sel"][b])
        assert int(g["sel_counts"][b]) == n, (what, b)
        assert np.array_equal(g["sel_index"][b, :n], r["sel"][b]) and (g["sel_index"][b, n:] == -1).all(), (what, b)
        assert np.array_equal(g["targets_after_nms"][b, :n], r["targets"][b]), (what, b)
        assert not g["targets_after_nms"][b, n:].any(), (what, b)
    ratios = {}
    stat = g["bbox_after_nms_class" if kw["mode"] == "classify" else "bbox_after_nms_rank"]
    for k, got in (("loss", g["loss"]), ("stat", float(stat))):
        tol = max(4 * (e[k] if e else 0.0), 4 * ulp32(r["loss"]))
        ratios[k] = abs(got - r["loss"]) / tol if tol else 0.0
        assert abs(got - r["loss"]) <= tol, (what, k, got, r["loss"], tol)
    for k in ("grad_acceptance", "grad_prob"):
        got, want = g[k], r[k]
        if want is None:
            assert got is None, (what, k)
            continue
        off = np.ones(want.shape[:2], bool)
        for b in range(B):
            off[b, r["sel"][b]] = False
        assert not got[off].any(), "%s: %s is not 0 off the selection" % (what, k)
        top = float(np.abs(want).max())
        tol = max(4 * (e[k] if e else 0.0), 4 * ulp32(top))
        d = float(np.abs(got.astype(np.float64) - want).max())
        ratios[k] = d / tol if tol else 0.0
        assert d <= tol, (what, k, d, tol, top)
    print("%s: |gpu - restatement| / tolerance: %s" % (what, " ".join("%s %.3f" % (k, v) for k, v in ratios.items())))
    return ratios


def golden_sample(cid, dev):
    from groomed_nms_amd import sampling
    c = H.case_of(cid)
    s = sampling.sample_anchors(_t(c["target_labels"], dev), _t(c["prob"], dev), _t(c["val_counts"], dev), box_samples=c["box_samples"],
                                fg_fraction=c["fg_fraction"])
    want = H.sampled(cid)
    fg_counts = s.fg_counts.cpu().numpy()
    for b, l in enumerate(want["fg_lists"]):
        assert fg_counts[b] == len(l) and np.array_equal(s.fg_index[b, :len(l)].cpu().numpy(), l)
    return s


@pytest.mark.parametrize("cid", H.case_ids())
def test_golden_cases(dev, cid):
    """every golden case by the rule; the cap case fails for any implementation that ranks only the selected boxes (the host test
    test_the_cap_case_tells_the_tail_apart shows the margin)"""
    c, r, e = H.case_of(cid), H.restated(cid), H.reference_errors(cid)
    g = run_gpu(dev, c, golden_sample(cid, dev), c["kw"])
    check(g, r, e, cid, c["kw"])
    # and against the reference itself
    for k, want in (("loss", float(c["loss"])), ("grad_acceptance", c["grad_acceptance"]), ("grad_prob", c["grad_prob"])):
        got = g[k]
        if got is None:
            assert not np.asarray(want).any(), (cid, k)
            continue
        top = float(np.abs(want).max())
        tol = max(8 * e[k], 4 * ulp32(top))           # |gpu - reference| <= |gpu - restatement| + e_ref
        assert float(np.abs(np.asarray(got, np.float64) - want).max()) <= tol, (cid, k)


def test_bit_for_bit_against_existing_entries(dev):
    """without a tail (fg_counts <= max_nms_boxes, mode rank): scores_after_nms == differentiable_nms_with_iou2d_batched on
    bbox_transform_inv(...) gathered at sel_index, and the per-image losses == ap_loss_batched on those"""
    import groomed_nms_amd as G
    from groomed_nms_amd import proposals
    from groomed_nms_amd.aploss import ap_loss_batched
    cid = "r210/reference"
    c = H.case_of(cid)
    loss, info, heads = call(dev, c, golden_sample(cid, dev), c["kw"])
    B, K = info["sel_index"].shape
    n = info["sel_counts"]
    assert int(n.min()) > 0 and int(n.max()) < K
    boxes = proposals.bbox_transform_inv(_t(c["rois"][0], dev), _t(c["bbox_2d"], dev), c["means"][:4], c["stds"][:4])
    idx = info["sel_index"].clamp(min=0)
    sel_boxes = torch.gather(boxes, 1, idx[:, :, None].expand(B, K, 4))
    sel_scores = torch.gather(heads["acceptance"].detach(), 1, idx)
    kw = c["kw"]
    prob = G.differentiable_nms_with_iou2d_batched(sel_scores, sel_boxes, counts=n, nms_threshold=kw["nms_threshold"], pruning_method=kw["pruning_method"],
                                                   temperature=kw["temperature"], valid_box_prob_threshold=kw["valid_box_prob_threshold"],
                                                   group_boxes=kw["group_boxes"], mask_group_boxes=kw["mask_group_boxes"], group_size=kw["group_size"])[0]
    losses = ap_loss_batched(prob, info["targets_after_nms"], counts=n)
    for b in range(B):
        assert torch.equal(prob[b, :int(n[b])], info["scores_after_nms"][b, :int(n[b])]), b
    assert torch.equal(losses, info["losses"])
    assert float(info["targets_after_nms"].sum()) > 0 and float(losses.max()) > 0


def _ap(lib, dev, lg, tg, counts=None, tail=None):
    from groomed_nms_amd._lib import ptr, check as chk, stream_ptr
    B, N = lg.shape
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty((B, N), dtype=torch.float32, device=dev)
    if tail is None:
        chk(lib.gnms_aploss(ptr(lg), ptr(tg), B, N, ptr(counts), 1.0, 0.0, ptr(loss), ptr(grad), stream_ptr()), "gnms_aploss")
    else:
        chk(lib.gnms_aploss_tail(ptr(lg), ptr(tg), B, N, ptr(counts), ptr(tail), 1.0, 0.0, ptr(loss), ptr(grad), stream_ptr()), "gnms_aploss_tail")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("N,E,lo", [(300, 200, -0.5), (700, 37, -0.5), (1500, 1000, -0.5), (2047, 1, -0.5), (300, 500, 1.5), (1100, 64, 0.2)])
def test_aploss_tail(dev, N, E, lo):
    """tail 0 == gnms_aploss bit for bit; tail E matches gnms_aploss on the same rows with E explicit zero-logit negatives appended (loss
    within 4 ulps, explicit gradients within 4 ulps of the largest); N + E crossing 2047 (the other route of gnms_aploss); a minimum
    positive above 1 (lo = 1.5) puts the tail outside the valid window: it changes nothing"""
    from groomed_nms_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(N * 7 + E)
    B = 3
    lg = rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32)
    tg = (rng.uniform(0, 1, (B, N)) < 0.15).astype(np.float32)
    lg[tg == 1] = rng.uniform(lo, lo + 1.5, int(tg.sum())).astype(np.float32)
    tg[:, ::17] = -1.0                                              # neither label: ignored
    counts = np.array([N, N - 5, max(1, N // 2)], np.int32)
    tails = np.array([E, E, max(E - 3, 0)], np.int32)
    LG, TG, C = _t(lg, dev), _t(tg, dev), _t(counts, dev)
    l0, g0 = _ap(lib, dev, LG, TG, C)
    l1, g1 = _ap(lib, dev, LG, TG, C, tail=_t(np.zeros(B, np.int32), dev))
    if N < 2048:                                                     # (from 2048 on gnms_aploss spreads the positives over the machine)
        assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    lt, gt = _ap(lib, dev, LG, TG, C, tail=_t(tails, dev))
    if lo > 1.0:
        assert np.array_equal(lt, l1) and np.array_equal(gt, g1)
    else:
        assert (lt[tails > 0] > l1[tails > 0]).all()                 # more negatives in the window: a lower precision
        assert np.array_equal(lt[tails == 0], l1[tails == 0])
    for b in range(B):                                               # explicit zeros appended, one image at a time (ragged rows)
        n, e = int(counts[b]), int(tails[b])
        row_l = np.concatenate([lg[b, :n], np.zeros(e, np.float32)])[None]
        row_t = np.concatenate([tg[b, :n], np.zeros(e, np.float32)])[None]
        le, ge = _ap(lib, dev, _t(row_l, dev), _t(row_t, dev))
        top = float(np.abs(ge[0, :n]).max())
        dl, dg = abs(float(lt[b]) - float(le[0])), float(np.abs(gt[b, :n] - ge[0, :n]).max())
        print("N %d E %d image %d: loss %.9g vs %.9g (%.2f ulps), gradient %.2f ulps of the largest" % (n, e, b, lt[b], le[0], dl / ulp32(le[0]),
                                                                                                      dg / ulp32(top)))
        assert dl <= 4 * ulp32(le[0]) and dg <= 4 * ulp32(top)
        assert not gt[b, n:].any()


def synthetic(counts, quota, K=64):
    """R = 210, B = 3 on the r210 grid: the 2D heads are shifts by multiples of 1/16 of the anchor with means 0 and stds 1, so the decoded
    boxes -- and with them the overlaps -- are the same numbers in float32 and float64 and the 4-ulp rule has something to hold on to"""
    c = dict(H.case_of("r210/reference"))
    rng = np.random.default_rng(sum(counts) + 11)
    ext = lambda a: np.concatenate([a, a[:1]], 0)           # noqa: E731  (a third image: the first one again, other heads below)
    for k in ("prob", "acceptance", "bbox_3d", "raw_gt", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor", "gts_val", "gts_3d", "val_counts"):
        c[k] = ext(c[k])
    B, R = 3, c["rois"].shape[1]
    c["rois"] = np.round(c["rois"])
    c["acceptance"] = rng.permutation(B * R).reshape(B, R).astype(np.float32) / np.float32(B * R) * np.float32(0.9) + np.float32(0.05)
    d2 = np.zeros((B, R, 4), np.float32)
    d2[:, :, :2] = rng.integers(-4, 5, (B, R, 2)).astype(np.float32) / 16
    c["bbox_2d"] = d2
    c["means"], c["stds"] = c["means"].copy(), c["stds"].copy()
    c["means"][:4], c["stds"][:4] = 0.0, 1.0
    c["val_counts"] = c["val_counts"].copy()
    fg = []
    for b, n in enumerate(counts):
        if n < 0:                                            # a skipped image: no valid ground truth, nothing sampled
            c["val_counts"][b] = 0
            n = 0
        fg.append(np.sort(rng.choice(R, n, replace=False)))
    kw = dict(c["kw"], max_nms_boxes=K)
    c["kw"] = kw
    return c, fg, [q if len(f) else 0 for q, f in zip(quota, fg)]


@pytest.mark.parametrize("counts,quota,mode", [((-1, 1, 63), (0, 1, 63), "rank"), ((64, 65, 150), (64, 65, 150), "rank"),
                                               ((65, 150, 20), (65, 0, 20), "rank"), ((0, 0, -1), (0, 0, 0), "rank"),
                                               ((64, 65, 150), (64, 65, 150), "rank_all"), ((150, 1, 0), (150, 1, 0), "classify"),
                                               ((0, 0, 0), (0, 0, 0), "classify")])
def test_synthetic_small_shapes(dev, counts, quota, mode):
    """max_nms_boxes = 64 with 0, 1, 63, 64, 65 and 150 sampled foreground anchors; a skipped image, an image with quota 0 (counted,
    contributes 0), a batch without any foreground (loss 0, gradients 0)"""
    c, fg, quota = synthetic(counts, quota)
    kw = dict(c["kw"], mode=mode)
    r = H.restate(c["prob"], c["acceptance"], c["bbox_2d"], c["bbox_3d"], c["raw_gt"], fg, quota, c["rois"], c["rois_3d"], c["rois_3d_cen"], c["p2"],
                  c["scale_factor"], c["gts_val"], c["gts_3d"], c["val_counts"], means=c["means"], stds=c["stds"], **kw)
    g = run_gpu(dev, c, sample_of(fg, quota, c["rois"].shape[1], dev), kw)
    check(g, r, None, "synthetic %s %s" % (counts, mode), kw)
    if sum(len(f) for f in fg) == 0:
        assert g["loss"] == 0.0 and not g["grad_acceptance"].any() and int(g["img_cnt"]) == 0


def test_row_strided_targets_and_upstream_gradient(dev):
    """raw_gt read in place from wider rows gives the same bits; an upstream gradient scales the stored gradients; two eager calls agree,
    also behind calls of other shapes that leave the allocator's blocks dirty.

    (Behind calls of another shape the one launch of the layer once took stale hand-off granules for this call's: DESIGN.md 3.16.)"""
    cid = "r210/class_confidence"
    c = H.case_of(cid)
    s = golden_sample(cid, dev)
    a = run_gpu(dev, c, s, c["kw"])
    b = run_gpu(dev, c, s, c["kw"])
    wide = torch.full(c["raw_gt"].shape[:2] + (40,), 7.0, device=dev)
    wide[:, :, 5:26] = _t(c["raw_gt"], dev)
    v = run_gpu(dev, c, s, c["kw"], views={"raw_gt": wide[:, :, 5:26]})
    u = run_gpu(dev, c, s, c["kw"], upstream=2.5)
    for k in ("loss", "grad_acceptance", "grad_prob", "scores_after_nms", "targets_after_nms", "sel_index"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], v[k]), k
    assert a["grad_prob"].any() and a["grad_acceptance"].any()
    for k in ("grad_acceptance", "grad_prob"):
        assert np.array_equal(u[k], a[k] * np.float32(2.5)), k


def test_graph_capture_behind_sample_anchors(dev):
    """sample_anchors + after_nms_loss + the backward in ONE graph, replayed on two new inputs: bit for bit the eager results.
    (A memset node in the chain made every replay after the first wrong: DESIGN.md 3.16.)"""
    from groomed_nms_amd import sampling, after_nms
    cid = "r210/reference"
    c = H.case_of(cid)
    kw = H.api_kw(c["kw"])
    t = {k: _t(c[k], dev) for k in ARRAYS + ("prob", "target_labels")}
    acc_data = _t(c["acceptance"], dev)

    def step():
        # (a leaf of the step's own: one kept across steps carries a gradient accumulator bound to the stream of its first use)
        acc = acc_data.detach().requires_grad_(True)
        s = sampling.sample_anchors(t["target_labels"], t["prob"], t["val_counts"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])
        loss, info = after_nms.after_nms_loss(t["prob"], acc, t["bbox_2d"], t["bbox_3d"], (None, t["raw_gt"]), s, t["rois"], t["rois_3d"],
                                              t["rois_3d_cen"], t["p2"], t["scale_factor"], t["gts_val"], t["gts_3d"], t["val_counts"],
                                              means=c["means"], stds=c["stds"], **kw)
        (ga,) = torch.autograd.grad(loss, acc)
        return loss, ga, info["scores_after_nms"], info["sel_index"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    rng = np.random.default_rng(3)
    for trial in range(2):
        new_acc = (rng.permutation(acc_data.numel()).reshape(acc_data.shape).astype(np.float32) + 1) / np.float32(acc_data.numel() + 1)
        new_b3 = c["bbox_3d"] + rng.normal(0, 0.01, c["bbox_3d"].shape).astype(np.float32)
        with torch.no_grad():
            acc_data.copy_(_t(new_acc, dev))
            t["bbox_3d"].copy_(_t(new_b3, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in out]
        want = step()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (trial, k)
        assert float(got[0].detach()) > 0 and bool(got[1].any())
