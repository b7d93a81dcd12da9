"""Anchor target assignment on the MI355X (csrc/targets.hip): the compute_targets drop-in, compute_targets_batched and iou_ign against
the reference's goldens and against the NumPy checker of test_targets_host.py.  Every comparison is exact (same dtype, same shape,
equal values, NaN where NaN)."""
import numpy as np
import pytest
import torch

from conftest import Golden
from test_targets_host import case_inputs, checker, same
from groomed_nms_amd.synthetic import anchor_scene as scene

pytestmark = pytest.mark.gpu

CASES = ["loss", "stats", "2d", "nodecomp", "vel16", "vel17", "vel17_anchors", "ign_only", "ign_only_3d", "empty", "no_ign", "no_ign_thresh0",
         "dups", "best_below_fg", "best0", "zero_area"]


@pytest.fixture(scope="module")
def T():
    from groomed_nms_amd import _lib, targets
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return targets


@pytest.fixture(scope="module")
def gold():
    return Golden("targets.npz")


def _drop_in_kwargs(kw):
    out = {k: v for k, v in kw.items() if v is not None}
    return out


@pytest.mark.parametrize("case", CASES)
def test_drop_in_matches_reference(T, gold, case):
    args, kw = case_inputs(gold, case)
    t, o, g = T.compute_targets(*args, **_drop_in_kwargs(kw))
    assert same(t, gold[case + "/transforms"])
    assert same(g, gold[case + "/raw_gt"])
    if gold.has(case + "/ols"):
        assert same(o, gold[case + "/ols"])
    else:
        assert o is None


def test_drop_in_accepts_the_default_anchors(T, gold):
    """lib/rpn_util.py:626 passes no anchors; the reference's default [] raises there, the drop-in reads it as no decomp / no velocity"""
    args, kw = case_inputs(gold, "2d")
    t, o, g = T.compute_targets(*args)
    assert same(t, gold["2d/transforms"]) and same(g, gold["2d/raw_gt"]) and same(o, gold["2d/ols"])


@pytest.mark.parametrize("case", [c for c in CASES if c not in ("empty", "no_ign", "no_ign_thresh0", "best_below_fg", "best0", "nodecomp",
                                                                "vel17_anchors")])
def test_iou_ign_matches_reference(T, gold, case):
    from groomed_nms_amd import overlaps
    args, _ = case_inputs(gold, case)
    assert same(overlaps.iou_ign(args[3], args[1]), gold[case + "/ols_ign"])


def _batched_one(T, args, kw, **extra):
    gts_val, gts_ign, lbls, rois = args[:4]
    dev = torch.device("cuda")
    M = len(gts_val)
    g3 = kw["gts_3d"]
    anchors = kw["anchors"]
    r = torch.from_numpy(np.ascontiguousarray(rois))[None].to(dev)
    return T.compute_targets_batched(
        r, torch.from_numpy(gts_val)[None].to(dev) if M else None, torch.from_numpy(lbls.astype(np.int32))[None].to(dev) if M else None,
        *args[4:], gts_ign=torch.from_numpy(gts_ign)[None].to(dev) if len(gts_ign) else None,
        gts_3d=torch.from_numpy(g3)[None].to(dev) if g3 is not None else None,
        rois_3d=torch.from_numpy(kw["rois_3d"])[None].to(dev) if kw["rois_3d"] is not None else None,
        rois_3d_cen=torch.from_numpy(kw["rois_3d_cen"])[None].to(dev) if kw["rois_3d_cen"] is not None else None,
        anchors=torch.from_numpy(anchors).to(dev) if anchors is not None else None,
        want=("transforms", "raw_gt", "ols_max", "ols", "ols_ign", "best_roi"), **extra)


@pytest.mark.parametrize("case", CASES)
def test_batched_matches_reference_and_checker(T, gold, case):
    args, kw = case_inputs(gold, case)
    res = _batched_one(T, args, kw)
    ref = checker(*args, **kw)
    assert same(res.transforms[0].cpu().numpy(), gold[case + "/transforms"])
    assert same(res.raw_gt[0].cpu().numpy(), gold[case + "/raw_gt"])
    if gold.has(case + "/ols"):
        assert same(res.ols[0].cpu().numpy(), gold[case + "/ols"])
        assert same(res.best_roi[0].cpu().numpy(), ref["best_roi"])
    if gold.has(case + "/ols_ign"):
        assert same(res.ols_ign[0].cpu().numpy(), gold[case + "/ols_ign"])
    assert same(res.ols_max[0].cpu().numpy(), ref["ols_max"].astype(np.float64))
    if gold.has(case + "/means"):
        n = _batched_one(T, args, kw, means=gold[case + "/means"], stds=gold[case + "/stds"])
        assert same(n.transforms[0].cpu().numpy(), gold[case + "/transforms_norm"])


def test_batched_3d_without_any_gt_row_writes_the_full_width(T, gold):
    """gts_3d [B, 0, 16] (no image has a valid GT, some have ignore boxes): the empty tensor reaches C as NULL, and the outputs must
    still be the 3D widths, every element written (the loss's padded gts_3d of a batch without valid GTs)"""
    args, kw = case_inputs(gold, "ign_only_3d")
    gts_ign, rois = args[1], args[3]
    d = torch.device("cuda")
    B, R = 2, rois.shape[0]
    rb = torch.from_numpy(np.stack([rois, rois]).astype(rois.dtype)).to(d)
    gi = torch.from_numpy(np.stack([gts_ign, np.full_like(gts_ign, np.nan)])).to(d)
    out = dict(transforms=torch.full((B, R, 23), float("nan"), device=d), raw_gt=torch.full((B, R, 21), float("nan"), device=d),
               ols_max=torch.full((B, R), float("nan"), dtype=torch.float64, device=d))
    res = T.compute_targets_batched(rb, torch.zeros((B, 0, 4), dtype=torch.float64, device=d), torch.zeros((B, 0), dtype=torch.int32, device=d),
                                    *args[4:], gts_ign=gi, ign_counts=torch.tensor([len(gts_ign), 0], dtype=torch.int32, device=d),
                                    gts_3d=torch.zeros((B, 0, 16), dtype=torch.float64, device=d), rois_3d=torch.from_numpy(np.stack([kw["rois_3d"]] * 2)).to(d),
                                    anchors=torch.from_numpy(kw["anchors"]).to(d), want=tuple(out), out=out)
    t, g = res.transforms.cpu().numpy(), res.raw_gt.cpu().numpy()
    assert t.shape == (B, R, 23) and g.shape == (B, R, 21)
    assert same(t[0], gold["ign_only_3d/transforms"]) and same(g[0], gold["ign_only_3d/raw_gt"])
    # image 1 has neither GTs nor ignore boxes: every row background (:518-521), all else zero
    ref1 = np.zeros((R, 23), np.float32)
    ref1[:, 4] = -1
    assert same(t[1], ref1) and same(g[1], np.zeros((R, 21), np.float32))
    assert not torch.isnan(res.ols_max).any()


# --- at scale: the reference's configuration (crop 512 x 1760, stride 16, 36 anchors: R = 126 720) ---------------------------------
TH = (0.5, 0.5, 0.0, 0.5, 0.35)


def run_scene(T, s, use_r3=True, means=None, stds=None, out=None, want=("transforms", "raw_gt", "ols_max", "best_roi")):
    d = torch.device("cuda")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)      # noqa: E731
    return T.compute_targets_batched(tt(s["rois"]), tt(s["gv"]), tt(s["lb"]), *TH, gts_ign=tt(s["gi"]), val_counts=tt(s["Mc"].astype(np.int32)),
                                     ign_counts=tt(s["Kc"].astype(np.int32)), gts_3d=tt(s["g3"]), rois_3d=tt(s["r3"]) if use_r3 else None,
                                     rois_3d_cen=tt(s["cen"]) if use_r3 else None, anchors=tt(s["anchors"]), means=means, stds=stds,
                                     want=want, out=out)


def check_scene(s, res, b, use_r3=True, means=None, stds=None):
    m, k = s["Mc"][b], s["Kc"][b]
    kw = dict(gts_3d=s["g3"][b, :m], anchors=s["anchors"], tracker=s["rois"][b][:, 4])
    if use_r3:
        kw.update(rois_3d=s["r3"][b], rois_3d_cen=s["cen"][b])
    ref = checker(s["gv"][b, :m], s["gi"][b, :k], s["lb"][b, :m], s["rois"][b], *TH, means=means, stds=stds, **kw)
    assert same(res.transforms[b].cpu().numpy(), ref["transforms"]), "transforms of image %d (M = %d, K = %d)" % (b, m, k)
    assert same(res.raw_gt[b].cpu().numpy(), ref["raw_gt"])
    assert same(res.ols_max[b].cpu().numpy(), ref["ols_max"].astype(np.float64))
    bro = res.best_roi[b].cpu().numpy()
    assert same(bro[:m], ref["best_roi"]) and (bro[m:] == -1).all()


@pytest.mark.parametrize("B", [2, 8])
def test_at_scale_ragged_with_garbage_padding(T, B):
    s = scene(np.random.default_rng(B), B)
    res = run_scene(T, s)
    torch.cuda.synchronize()
    for b in range(B):
        check_scene(s, res, b)


def test_at_scale_float64_rois_through_anchors(T):
    s = scene(np.random.default_rng(11), 2, Mmax=64, dtype=np.float64, D3=17, acols=12)
    res = run_scene(T, s, use_r3=False)
    for b in range(2):
        check_scene(s, res, b, use_r3=False)


def test_fused_normalisation_is_the_call_sites_numpy(T):
    rng = np.random.default_rng(5)
    s = scene(rng, 2, Mmax=48)
    means, stds = rng.normal(0, 0.1, (1, 13)), rng.uniform(0.1, 2, (1, 13))
    res = run_scene(T, s, means=means, stds=stds)
    plain = run_scene(T, s)
    for b in range(2):
        t = plain.transforms[b].cpu().numpy()             # lib/loss/rpn_3d.py:440-447, in place on float32
        t[:, 0:4] -= means[:, 0:4]
        t[:, 0:4] /= stds[:, 0:4]
        t[:, 5:14] -= means[:, 4:13]
        t[:, 5:14] /= stds[:, 4:13]
        assert same(res.transforms[b].cpu().numpy(), t)
        check_scene(s, res, b, means=means, stds=stds)


def test_outputs_prefilled_with_nan_come_back_fully_written(T):
    s = scene(np.random.default_rng(3), 2, Mmax=32)
    B, R = s["rois"].shape[:2]
    d = torch.device("cuda")
    out = dict(transforms=torch.full((B, R, 23), float("nan"), device=d), raw_gt=torch.full((B, R, 21), float("nan"), device=d),
               ols_max=torch.full((B, R), float("nan"), dtype=torch.float64, device=d),
               ols=torch.full((B, R, 32), float("nan"), dtype=torch.float64, device=d),
               ols_ign=torch.full((B, R, 8), float("nan"), dtype=torch.float64, device=d),
               best_roi=torch.full((B, 32), 12345, dtype=torch.int64, device=d))
    res = run_scene(T, s, out=out, want=tuple(out))
    fresh = run_scene(T, s, want=tuple(out))
    for name in out:
        a, f = getattr(res, name), getattr(fresh, name)
        assert a.data_ptr() == out[name].data_ptr()
        assert torch.equal(a, f) or same(a.cpu().numpy(), f.cpu().numpy()), name
    assert not torch.isnan(res.transforms).any() and not torch.isnan(res.raw_gt).any()
    assert (res.best_roi != 12345).all()


def test_graph_replay_equals_eager(T):
    s = scene(np.random.default_rng(7), 2, Mmax=24)
    d = torch.device("cuda")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)      # noqa: E731
    ins = dict(rois=tt(s["rois"]), gv=tt(s["gv"]), lb=tt(s["lb"]), gi=tt(s["gi"]), vc=tt(s["Mc"].astype(np.int32)), ic=tt(s["Kc"].astype(np.int32)),
               g3=tt(s["g3"]), r3=tt(s["r3"]), cen=tt(s["cen"]), anchors=tt(s["anchors"]))
    means, stds = np.full(13, 0.01), np.full(13, 0.5)

    def call():
        return T.compute_targets_batched(ins["rois"], ins["gv"], ins["lb"], *TH, gts_ign=ins["gi"], val_counts=ins["vc"], ign_counts=ins["ic"],
                                         gts_3d=ins["g3"], rois_3d=ins["r3"], rois_3d_cen=ins["cen"], anchors=ins["anchors"], means=means,
                                         stds=stds, want=("transforms", "raw_gt", "ols_max", "ols", "best_roi"))
    eager = call()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()                                                           # warm-up outside capture
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = call()
    for _ in range(2):
        for name in ("transforms", "raw_gt", "ols_max", "ols"):
            getattr(cap, name).fill_(float("nan"))
        cap.best_roi.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        for name in cap._fields:
            a, e = getattr(cap, name), getattr(eager, name)
            if e is not None:
                assert same(a.cpu().numpy(), e.cpu().numpy()), name


def test_two_streams_equal_serial(T):
    s1 = scene(np.random.default_rng(21), 2, Mmax=40)
    s2 = scene(np.random.default_rng(22), 2, Mmax=200)
    serial = [run_scene(T, s1), run_scene(T, s2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    for i, (s, st) in enumerate(zip((s1, s2), streams)):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs[i] = run_scene(T, s)
    torch.cuda.synchronize()
    for a, b in zip(outs, serial):
        for name in ("transforms", "raw_gt", "ols_max", "best_roi"):
            assert same(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name


def test_more_than_256_ground_truths_is_unsupported(T):
    from groomed_nms_amd import _lib
    d = torch.device("cuda")
    rois = torch.zeros((1, 64, 5), device=d)
    gv = torch.zeros((1, 257, 4), dtype=torch.float64, device=d)
    lb = torch.ones((1, 257), dtype=torch.int32, device=d)
    with pytest.raises(_lib.GnmsError, match=r"\(-2\)"):
        T.compute_targets_batched(rois, gv, lb, *TH)
    with pytest.raises(_lib.GnmsError, match=r"\(-2\)"):
        T.compute_targets_batched(rois, None, None, *TH, gts_ign=torch.zeros((1, 257, 4), dtype=torch.float64, device=d))
