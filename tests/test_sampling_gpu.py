"""GPU tests of the anchor sampler and the weighted classification term (groomed_nms_amd/sampling.py, csrc/sampling.hip) against the
reference's goldens (tests/golden/sampling.npz) and the float64 restatement of tests/test_sampling_host.py.

Measured |gpu - float64 restatement| / e_ref per golden case: DESIGN.md 3.14 (each test prints its figures before it asserts)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sampling_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_gpu(dev, target_labels, prob, val_counts, cls, *, box_samples, fg_fraction, focal_loss=0, cls_2d_lambda=1, upstream=None):
    """both calls and the backward; everything back on the host as NumPy"""
    from groomed_nms_amd import sampling
    x = _t(cls, dev).requires_grad_(True)
    s = sampling.sample_anchors(_t(target_labels, dev), _t(prob, dev), _t(val_counts, dev) if val_counts is not None else None,
                                box_samples=box_samples, fg_fraction=fg_fraction)
    loss, stats = sampling.classification_loss(x, s, fg_fraction=fg_fraction, focal_loss=focal_loss, cls_2d_lambda=cls_2d_lambda)
    (loss if upstream is None else loss * upstream).backward()
    torch.cuda.synchronize()
    out = {k: getattr(s, k).cpu().numpy() for k in ("labels", "labels_scores", "bbox_weights", "fg_index", "fg_counts", "counts",
                                                    "sampled", "labels_weight")}
    out.update(loss=float(loss.detach().cpu()), grad=x.grad.cpu().numpy(), acc_fg=float(stats["acc_fg"].cpu()),
               acc_bg=float(stats["acc_bg"].cpu()), cls=float(stats["cls"].cpu()))
    return out


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def check_sampler(g, r):
    """the sampler's outputs against the restatement: all exact"""
    assert np.array_equal(g["sampled"], r["enc"])
    assert np.array_equal(g["labels"], r["labels"])
    assert np.array_equal(g["bbox_weights"], r["bbox_weights"])
    assert np.array_equal(g["labels_scores"], r["labels_scores"], equal_nan=True)
    assert np.array_equal(g["counts"], r["counts"])
    for b, want in enumerate(r["fg_lists"]):
        n = int(g["fg_counts"][b])
        assert n == len(want) and np.array_equal(g["fg_index"][b, :n], want)
        assert (g["fg_index"][b, n:] == -1).all()


def check_weights(g, r, focal_loss):
    if not focal_loss:
        assert np.array_equal(g["labels_weight"].view(np.int32), r["labels_weight"].view(np.int32)), "labels_weight is not bit-equal"
    else:       # the device's float64 pow may differ from libm's in its last bit: a float32 moves only at a rounding boundary
        d = np.abs(g["labels_weight"].view(np.int32).astype(np.int64) - r["labels_weight"].view(np.int32).astype(np.int64))
        print("labels_weight: %d of %d differ by one float32 ulp" % (int((d == 1).sum()), d.size))
        assert d.max() <= 1


def check_loss(g, r, e_loss, e_grad, what):
    d_loss = abs(g["loss"] - r["loss"])
    d_grad = float(np.abs(g["grad"].astype(np.float64) - r["grad"]).max())
    gmax = float(np.abs(r["grad"]).max())
    print("%s: loss |gpu - f64| = %.3e (e_ref %.3e, ratio %s, %.2f ulp); grad %.3e (e_ref %.3e, ratio %s, %.2f ulp of the largest entry)"
          % (what, d_loss, e_loss, "%.2f" % (d_loss / e_loss) if e_loss else "-", d_loss / ulp32(r["loss"]) if r["loss"] else 0.0,
             d_grad, e_grad, "%.2f" % (d_grad / e_grad) if e_grad else "-", d_grad / ulp32(gmax) if gmax else 0.0))
    assert d_loss <= max(4 * e_loss, 4 * ulp32(r["loss"]))
    assert d_grad <= max(4 * e_grad, 4 * ulp32(gmax))
    assert g["cls"] == g["loss"]


@pytest.mark.parametrize("cid", H.case_ids())
def test_reference_goldens(dev, cid):
    c, r = H.case_of(cid), H.restated(cid)
    e_loss, e_grad = H.reference_errors(cid)
    g = run_gpu(dev, c["target_labels"], c["prob"], c["val_counts"], c["cls"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"],
                focal_loss=c["focal_loss"])
    sampled_ref = (c["grad"] != 0).any(axis=2)                   # the reference's sampled set
    assert np.array_equal(g["labels_weight"] != 0, sampled_ref)
    check_sampler(g, r)
    assert g["acc_fg"] == c["stats"][0] and g["acc_bg"] == c["stats"][1]
    check_weights(g, r, c["focal_loss"])
    check_loss(g, r, e_loss, e_grad, cid)
    # and against the reference itself, with the two errors added
    assert abs(g["loss"] - float(c["loss"])) <= e_loss + max(4 * e_loss, 4 * ulp32(r["loss"]))
    assert (g["grad"][~sampled_ref] == 0).all()


def tie_scene(rng, R=1332, nan=0):
    """background probabilities drawn from eight values: every cut falls inside a run of equal keys"""
    B, C = 2, 4
    t = -np.ones((B, R), np.float32)
    for b in range(B):
        t[b, rng.choice(R, 40, replace=False)] = rng.integers(1, C, 40)
        t[b, rng.choice(R, 60, replace=False)] = 0
    cls = rng.normal(0, 1.5, (B, R, C)).astype(np.float32)
    prob = torch.softmax(torch.from_numpy(cls), dim=2).numpy()
    prob[:, :, 0] = rng.choice(np.linspace(0.1, 0.8, 8).astype(np.float32), (B, R))
    if nan:
        for b in range(B):
            prob[b, rng.choice(R, nan, replace=False), 0] = np.nan
    return t, prob, cls


def test_tie_rule(dev):
    rng = np.random.default_rng(77)
    t, prob, cls = tie_scene(rng)
    kw = dict(box_samples=0.25, fg_fraction=0.5)
    g = run_gpu(dev, t, prob, np.array([3, 1], np.int32), cls, **kw)
    g2 = run_gpu(dev, t, prob, np.array([3, 1], np.int32), cls, **kw)
    for k in g:
        assert np.array_equal(g[k], g2[k], equal_nan=True), "%s differs between two runs" % k
    R = t.shape[1]
    for b in range(2):
        bg = np.flatnonzero(t[b] < 0)
        n_fg = int((t[b] > 0).sum())
        fg_num = min(round(R * 0.25 * 0.5), n_fg)
        quota = min(round(R * 0.25 - fg_num), len(bg))
        assert 0 < quota < len(bg)
        keys = prob[b, bg, 0]
        cutv = np.sort(keys)[quota - 1]
        assert np.sort(keys)[quota] == cutv                       # the cut is inside a run of equal keys
        sel = g["sampled"][b, bg] == 2
        assert int(sel.sum()) == quota and g["counts"][b, 5] == quota
        assert sel[keys < cutv].all() and not sel[keys > cutv].any()
        eq = np.flatnonzero(keys == cutv)
        k = int(sel[eq].sum())
        assert 0 < k < len(eq) and sel[eq[:k]].all() and not sel[eq[k:]].any()      # the lowest-indexed of the equal ones
    check_sampler(g, H.restate(t, prob, np.array([3, 1]), **kw))


def test_nan_keys_are_taken_last(dev):
    rng = np.random.default_rng(78)
    t, prob, cls = tie_scene(rng, nan=900)                        # more NaN keys than the background that is left out
    kw = dict(box_samples=0.8, fg_fraction=0.02)
    g = run_gpu(dev, t, prob, None, cls, **kw)
    r = H.restate(t, prob, None, cls, **kw)
    assert (r["counts"][:, 5] < r["counts"][:, 1]).all()
    for b in range(2):
        bg = t[b] < 0
        nan_sel = g["sampled"][b][bg & np.isnan(prob[b, :, 0])] == 2
        assert nan_sel.any() and not nan_sel.all()                # the cut falls among the NaN keys
        assert (g["sampled"][b][bg & ~np.isnan(prob[b, :, 0])] == 2).all()
    check_sampler(g, r)
    assert np.array_equal(g["labels_weight"].view(np.int32), r["labels_weight"].view(np.int32))


def test_full_width_once(dev):
    """the loss's call site: B = 2, R = 32 * 110 * 36, C = 4, box_samples = fg_fraction = 0.2, about 1 % foreground"""
    rng = np.random.default_rng(126720)
    B, R, C = 2, 126720, 4
    u = rng.random((B, R))
    t = -np.ones((B, R), np.float32)
    t[u < 0.01] = rng.integers(1, C, int((u < 0.01).sum()))
    t[(u >= 0.01) & (u < 0.04)] = 0
    cls = rng.normal(0, 2.0, (B, R, C)).astype(np.float32)
    prob = torch.softmax(torch.from_numpy(cls), dim=2).numpy()
    kw = dict(box_samples=0.2, fg_fraction=0.2, focal_loss=0)
    g = run_gpu(dev, t, prob, np.array([5, 9], np.int32), cls, **kw)
    r = H.restate(t, prob, np.array([5, 9]), cls, **kw)
    assert (r["counts"][:, 4] == r["counts"][:, 0]).all() and (r["counts"][:, 5] < r["counts"][:, 1]).all()
    check_sampler(g, r)
    check_weights(g, r, 0)
    assert g["acc_fg"] == r["acc_fg"] and g["acc_bg"] == r["acc_bg"]
    check_loss(g, r, 0.0, 0.0, "full width")


def test_select_topk_takes_the_sampled_foreground(dev):
    """fg_index / fg_counts go into proposals.select_topk unchanged (lib/loss/rpn_3d.py:731-737)"""
    from groomed_nms_amd import sampling, proposals
    c = H.case_of("r1332/both_cut")
    prob = _t(c["prob"], dev)
    s = sampling.sample_anchors(_t(c["target_labels"], dev), prob, _t(c["val_counts"], dev), box_samples=c["box_samples"],
                                fg_fraction=c["fg_fraction"])
    scores = prob[:, :, 1:].max(dim=2)[0].contiguous()
    K = 20
    idx, num, ssel, _ = proposals.select_topk(scores, K, candidates=s.fg_index, candidate_counts=s.fg_counts)
    torch.cuda.synchronize()
    r = H.restated("r1332/both_cut")
    for b in range(2):
        fg = r["fg_lists"][b]
        sc = scores[b].cpu().numpy()[fg]
        want = fg[np.argsort(-sc, kind="stable")][:K]
        n = int(num[b])
        assert n == min(K, len(fg)) and np.array_equal(idx[b, :n].cpu().numpy(), want)


def test_backward_scales_the_stored_gradient(dev):
    c = H.case_of("r210/both_cut_focal2")
    kw = dict(box_samples=c["box_samples"], fg_fraction=c["fg_fraction"], focal_loss=2)
    g1 = run_gpu(dev, c["target_labels"], c["prob"], c["val_counts"], c["cls"], **kw)
    g3 = run_gpu(dev, c["target_labels"], c["prob"], c["val_counts"], c["cls"], upstream=-3.0, **kw)
    assert np.abs(g1["grad"]).max() > 0
    assert np.array_equal(g3["grad"], g1["grad"] * np.float32(-3.0))
    # cls_2d_lambda scales the term in float32; 0 switches it off
    g0 = run_gpu(dev, c["target_labels"], c["prob"], c["val_counts"], c["cls"], cls_2d_lambda=0, **kw)
    assert g0["loss"] == 0.0 and not g0["grad"].any() and np.array_equal(g0["labels_weight"], g1["labels_weight"])
    gh = run_gpu(dev, c["target_labels"], c["prob"], c["val_counts"], c["cls"], cls_2d_lambda=0.5, **kw)
    assert gh["loss"] == np.float32(g1["loss"]) * np.float32(0.5)


def test_graph_capture_and_replay(dev):
    from groomed_nms_amd import sampling
    a, b = H.case_of("r1332/both_cut_focal2"), H.case_of("r1332/no_gt_image")
    kw = dict(box_samples=a["box_samples"], fg_fraction=a["fg_fraction"])
    assert kw == dict(box_samples=b["box_samples"], fg_fraction=b["fg_fraction"])
    st = {k: _t(a[k], dev) for k in ("target_labels", "prob", "val_counts", "cls")}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                  # warm-up outside the capture
        s = sampling.sample_anchors(st["target_labels"], st["prob"], st["val_counts"], **kw)
        sampling.classification_loss(st["cls"], s, fg_fraction=kw["fg_fraction"], focal_loss=2)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = sampling.sample_anchors(st["target_labels"], st["prob"], st["val_counts"], **kw)
        loss, stats = sampling.classification_loss(st["cls"], s, fg_fraction=kw["fg_fraction"], focal_loss=2)
    for k in st:                                                   # fresh inputs, then replay
        st[k].copy_(_t(b[k], dev))
    graph.replay()
    torch.cuda.synchronize()
    e = run_gpu(dev, b["target_labels"], b["prob"], b["val_counts"], b["cls"], focal_loss=2, **kw)
    for k in ("labels", "labels_scores", "bbox_weights", "fg_index", "fg_counts", "counts", "sampled", "labels_weight"):
        assert np.array_equal(getattr(s, k).cpu().numpy(), e[k]), k
    assert float(loss.cpu()) == e["loss"] and float(stats["acc_fg"].cpu()) == e["acc_fg"] and float(stats["acc_bg"].cpu()) == e["acc_bg"]


def test_non_default_stream_and_strided_label_column(dev):
    """on a side stream, with the label column read in place from rows of 21 floats (Targets.transforms[..., 4])"""
    from groomed_nms_amd import sampling
    c = H.case_of("r210/bg_cut")
    r = H.restated("r210/bg_cut")
    rows = torch.full((2, 210, 21), 7.0, device=dev)
    rows[:, :, 4] = _t(c["target_labels"], dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        x = _t(c["cls"], dev).requires_grad_(True)
        s = sampling.sample_anchors(rows[..., 4], _t(c["prob"], dev), _t(c["val_counts"], dev), box_samples=c["box_samples"],
                                    fg_fraction=c["fg_fraction"])
        loss, _ = sampling.classification_loss(x, s, fg_fraction=c["fg_fraction"])
        loss.backward()
    side.synchronize()
    assert np.array_equal(s.sampled.cpu().numpy(), r["enc"]) and np.array_equal(s.labels.cpu().numpy(), r["labels"])
    assert np.array_equal(s.labels_weight.cpu().numpy().view(np.int32), r["labels_weight"].view(np.int32))
    e_loss, e_grad = H.reference_errors("r210/bg_cut")
    check_loss(dict(loss=float(loss.detach().cpu()), cls=float(loss.detach().cpu()), grad=x.grad.cpu().numpy()), r, e_loss, e_grad, "side stream")


def test_argument_errors_return_their_codes(dev):
    from groomed_nms_amd import sampling, _lib
    lib = _lib.load()
    t = torch.zeros((2, 64), device=dev)
    with pytest.raises(_lib.GnmsError, match="C = 1"):
        sampling.sample_anchors(t, torch.ones((2, 64, 1), device=dev), None, box_samples=0.2, fg_fraction=0.2)
    with pytest.raises(_lib.GnmsError, match="R = 0"):
        sampling.sample_anchors(t[:, :0], torch.ones((2, 0, 4), device=dev), None, box_samples=0.2, fg_fraction=0.2)
    with pytest.raises(ValueError):
        sampling.sample_anchors(t, torch.ones((2, 64, 4), device=dev), None, box_samples=0.2, fg_fraction=None)
    with pytest.raises(NotImplementedError):
        sampling.sample_anchors(t, torch.ones((2, 64, 4), device=dev), None, box_samples=0.2, fg_fraction=0.2, hard_negatives=False)
    p = torch.full((2, 64, 4), 0.25, device=dev)
    s = sampling.sample_anchors(t - 1, p, None, box_samples=0.2, fg_fraction=0.2)
    with pytest.raises(ValueError):
        sampling.classification_loss(torch.zeros((2, 32, 4), device=dev), s, fg_fraction=0.2)
    # null outputs and a short workspace through the C ABI
    o = [s.labels, s.bbox_weights, s.labels_scores, s.sampled, s.fg_index, s.fg_counts, s.counts]
    ws = torch.empty(lib.gnms_sample_anchors_workspace_bytes(2, 64), dtype=torch.uint8, device=dev)
    args = lambda outs, nbytes: (t.data_ptr(), 1, p.data_ptr(), None, 2, 64, 4, 0.2, 1, 0.2, *[x.data_ptr() if x is not None else None for x in outs],  # noqa: E731
                                 ws.data_ptr(), nbytes, None)
    assert lib.gnms_sample_anchors(*args(o[:3] + [None] + o[4:], ws.numel())) == -1
    assert lib.gnms_sample_anchors(*args(o, ws.numel() - 1)) == -4
    torch.cuda.synchronize()
    assert lib.gnms_sample_anchors(*args(o, ws.numel())) == 0
    torch.cuda.synchronize()
