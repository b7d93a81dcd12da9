"""GPU tests of the loss module (groomed_nms_amd/loss.py, csrc/loss.hip) against tests/golden/loss.npz and the restatements of
tests/test_loss_module_host.py.

gnms_gt_filter is bit-exact against restate_gt_filter.  The module, through the reference's call signature: |gpu - restatement| <=
max(4 e, 4 float32 ulps of the value; for a gradient: of its largest entry) with e = |reference - restatement| of the same quantity as
the generator stored it, and |gpu - reference| <= max(8 e, 4 ulps) (DESIGN.md 3.14's rule, as the sibling GPU tests apply it).  The
gradients equal those of the five public calls composed by hand and differentiated by autograd, bit for bit.  Each test prints its
figures before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_loss_module_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
HEADS = ("cls", "prob", "bbox_2d", "bbox_3d", "acceptance")


@pytest.fixture(scope="module")
def dev():
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def imobjs_of(c):
    """the objects the records were written from (a class of ilbls comes back as "Van", a class of neither list as "Bus")"""
    out = []
    for b in range(len(c["counts"])):
        gts = []
        for row in c["records"][b, :int(c["counts"][b])]:
            k = int(row[20])
            gts.append(H.AttrDict(cls=H.LBLS[k - 1] if k > 0 else ("Van" if k == 0 else "Bus"), ign=bool(row[21]), visibility=float(row[22]),
                                  trunc=float(row[23]), bbox_full=row[0:4].copy(), bbox_3d=row[4:20].copy()))
        out.append(H.AttrDict(gts=gts, p2=c["p2"][b].copy(), scale_factor=float(c["scale_factor"][b])))
    return out


def one_image(c, b=0):
    """a case cut down to image b (B = 1)"""
    d = dict(c)
    for k in HEADS + ("p2", "scale_factor", "records", "counts", "transforms", "raw_gt"):
        d[k] = c[k][b:b + 1]
    return d


def leaves_of(c, dev, no_grad=()):
    x = {k: _t(c[k], dev).requires_grad_(k not in no_grad) for k in HEADS}
    x["acceptance"] = x["acceptance"].detach().unsqueeze(2).requires_grad_(True) if c["has_acceptance"] else None
    return x


def grids_of(c, dev):
    B = c["prob"].shape[0]
    return [_t(np.array(np.broadcast_to(c[k][None], (B,) + c[k].shape)), dev) for k in ("rois", "rois_3d", "rois_3d_cen")]


def run_module(dev, c, backward="backward", upstream=None, no_grad=(), module=None):
    """RPN_3D_loss(conf)(...) through the reference's call signature and the backward -> everything on the host, and the module"""
    from groomed_nms_amd.loss import RPN_3D_loss
    m = module or RPN_3D_loss(H.conf_of(c), verbose=True)
    x = leaves_of(c, dev, no_grad)
    rois, r3, cen = grids_of(c, dev)
    loss, stats = m(x["cls"], x["prob"], x["bbox_2d"], x["bbox_3d"], imobjs_of(c), [0, 0], rois=rois, rois_3d=r3, rois_3d_cen=cen,
                    bbox_acceptance_prob=x["acceptance"])
    wrt = [k for k in HEADS if x[k] is not None and x[k].requires_grad]
    if backward == "backward":
        (loss if upstream is None else loss * upstream).backward()
        grads = {k: x[k].grad for k in wrt}
    else:                                            # torch.autograd.grad with a device scalar
        grads = dict(zip(wrt, torch.autograd.grad(loss, [x[k] for k in wrt], grad_outputs=upstream)))
    torch.cuda.synchronize()
    out = {"total": float(loss.detach().cpu()), "vector": m.last_stats.cpu().numpy(), "list": stats}
    out["stats"] = {key: float(s["val"].cpu()) for s, (_, key) in zip(stats, m.stat_entries())}
    for k in HEADS:
        g = grads.get(k)
        out["grad_" + k] = g.cpu().numpy().reshape(c[k].shape) if g is not None else None
    return out, m


def check_against(g, r, e, what, factor, ref=None):
    """the rule: per quantity |gpu - want| <= max(factor * e, 4 ulps); want: the restatement's, or the reference's values `ref`"""
    ratios = {}
    for k, got in g["stats"].items():
        want = r["stats"][k] if ref is None else ref[k]
        if want is None:
            continue
        tol = max(factor * e[k], 4 * H.ulp32(want))
        ratios[k] = abs(got - want) / tol
        assert abs(got - want) <= tol, (what, k, got, want, tol)
    want = r["stats"]["total"] if ref is None else ref["total"]
    assert abs(g["total"] - want) <= max(factor * e["total"], 4 * H.ulp32(want)), (what, "total", g["total"], want)
    for k in H.GRADS:
        got, want = g[k], (r[k] if ref is None else ref[k])
        if got is None:
            assert want is None or not np.asarray(want).any() or k == "grad_acceptance", (what, k)
            continue
        if want is None:
            want = np.zeros(got.shape)
        top = float(np.abs(want).max())
        tol = max(factor * e[k], 4 * H.ulp32(top))
        d = float(np.abs(got.astype(np.float64) - want).max())
        ratios[k] = d / tol if tol else 0.0
        assert d <= tol, (what, k, d, tol, top)
    print("%s: |gpu - %s| / tolerance: %s" % (what, "restatement" if ref is None else "reference", " ".join("%s %.3f" % kv for kv in ratios.items())))


# ---------------------------------------------------------------------------------------------- gnms_gt_filter

def gt_filter(dev, records, counts, min_gt_vis, min_gt_h, use_trunc=False):
    """the entry alone, into buffers prefilled with 0xff bytes -> the six arrays on the host"""
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import ptr, check, stream_ptr
    lib = _lib.load()
    B, cap = records.shape[:2]
    rec, cnt = _t(records, dev), _t(counts.astype(np.int32), dev)
    shapes = dict(gts_val=((B, cap, 4), torch.float64), box_lbls=((B, cap), torch.int32), gts_3d=((B, cap, 16), torch.float64),
                  gts_ign=((B, cap, 4), torch.float64), val_counts=((B,), torch.int32), ign_counts=((B,), torch.int32))
    out = {}
    for k, (shape, dtype) in shapes.items():
        raw = torch.full((int(np.prod(shape)) * (8 if dtype == torch.float64 else 4),), 0xff, dtype=torch.uint8, device=dev)
        out[k] = raw.view(dtype).view(shape)
    check(lib.gnms_gt_filter(ptr(rec), ptr(cnt), B, cap, float(min_gt_vis), float(min_gt_h), 10e10, int(use_trunc), ptr(out["gts_val"]),
                             ptr(out["box_lbls"]), ptr(out["gts_3d"]), ptr(out["gts_ign"]), ptr(out["val_counts"]), ptr(out["ign_counts"]),
                             stream_ptr(dev)), "gnms_gt_filter")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(got, want, what):
    for k in ("gts_val", "box_lbls", "gts_3d", "gts_ign", "val_counts", "ign_counts"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)


def _scene_cases():
    """one case per stored scene (and min_gt_h)"""
    seen = {}
    for cid in H.case_ids():
        c = H.case_of(cid)
        seen.setdefault((cid.split("/")[0], str(c["scene"]), c["min_gt_h"]), cid)
    return sorted(seen.values())


@pytest.mark.parametrize("cid", _scene_cases())
def test_gt_filter_golden_scenes(dev, cid):
    c = H.case_of(cid)
    got = gt_filter(dev, c["records"], c["counts"], 0.65, c["min_gt_h"])
    same_bits(got, H.restate_gt_filter(c["records"], c["counts"], 0.65, c["min_gt_h"]), cid)


PATTERNS = ("all_removed", "all_ignored", "alternating", "last_valid", "mixed")


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 256])
def test_gt_filter_synthetic_counts(dev, count):
    """capacity 256, one image per pattern: wave and workgroup edges, stable order by a distinct marker (the first 3D column carries
    the row's index), padding rows zero in buffers that held 0xff bytes; use_trunc on the same rows"""
    rng = np.random.default_rng(count)
    cap, B = 256, len(PATTERNS)
    rec = np.zeros((B, cap, 24))
    rec[:, :, 0:4] = rng.uniform(1, 300, (B, cap, 4))
    rec[:, :, 4:20] = rng.normal(0, 5, (B, cap, 16))
    rec[:, :, 4] = np.arange(cap)[None] + 1000.0                      # the marker
    rec[:, :, 20] = rng.integers(1, 4, (B, cap))
    rec[:, :, 22], rec[:, :, 23] = 1.0, rng.uniform(0, 0.7, (B, cap))
    i = np.arange(cap)
    rec[0, :, 20] = -1
    rec[1, :, 21] = 1
    rec[2, i % 2 == 1, 22] = 0.5
    rec[3, :, 20] = 0
    rec[3, max(count - 1, 0), 20] = 2
    rec[3, :, 3], rec[3, :, 23] = 50.0, 0.0
    rec[4, :, 20] = rng.integers(-1, 4, cap)
    rec[4, :, 21] = rng.integers(0, 2, cap)
    rec[4, :, 22] = rng.uniform(0.4, 1.0, cap)
    rec[4, :, 3] = rng.uniform(5, 40, cap)
    rec[:, count:] = np.nan                                           # rows behind the count must not be read as ground truths
    counts = np.full(B, count, np.int32)
    for use_trunc in (False, True):
        want = H.restate_gt_filter(np.nan_to_num(rec), counts, 0.65, 12.0, use_trunc=use_trunc)
        got = gt_filter(dev, rec, counts, 0.65, 12.0, use_trunc=use_trunc)
        same_bits(got, want, (count, use_trunc))
        for b in range(B):
            nv = int(got["val_counts"][b])
            marks = got["gts_3d"][b, :nv, 0]
            assert (np.diff(marks) > 0).all() and np.array_equal(marks, 1000.0 + np.flatnonzero(~want["igns"][b] & ~want["rmvs"][b])), (count, b)
            assert not got["gts_val"][b, nv:].any() and not got["gts_ign"][b, int(got["ign_counts"][b]):].any()
    assert got["val_counts"][0] == 0 and got["ign_counts"][0] == 0 and got["val_counts"][1] == 0 and got["ign_counts"][1] == count
    assert got["val_counts"][3] == min(count, 1)


# ---------------------------------------------------------------------------------------------- the module

@pytest.mark.parametrize("cid", H.case_ids())
def test_module_golden_cases(dev, cid):
    c, r, e = H.case_of(cid), H.restated(cid), H.stored_errors(cid)
    g, m = run_module(dev, c)
    # the ground truths went through pack_ground_truths, the upload and gnms_gt_filter
    for k, v in m.last_ground_truths.items():
        assert np.array_equal(v.cpu().numpy(), r["gt"][k]), (cid, k)
    assert [s["name"] for s in g["list"]] == c["stat_names"]
    for s in g["list"]:
        assert s["val"].dim() == 0 and s["val"].dtype == torch.float64 and s["val"].device == dev
        assert s["val"].untyped_storage().data_ptr() == m.last_stats.untyped_storage().data_ptr()
    assert g["stats"]["total"] == g["total"] == float(np.float32(g["vector"][16]))
    check_against(g, r, e, cid, 4)
    check_against(g, r, e, cid, 8, ref=H.reference_values(c))
    assert not g["grad_bbox_3d"][:, :, 10:].any()
    if c["has_acceptance"]:                          # the running weight after its first step is the one the step used (`un` is held to the rule above)
        assert m.un_state.cpu().tolist() == [1.0, g["vector"][17]] and g["vector"][17] > 0
    else:
        assert g["grad_acceptance"] is None and m.un_state is None


def hand_composition(dev, c, x):
    """the five public calls as INTEGRATION.md composed them before the module, differentiated by autograd -> (loss, the regression's stats)"""
    from groomed_nms_amd import targets, sampling, regression, after_nms
    conf = H.conf_of(c)
    gt = H.restate_gt_filter(c["records"], c["counts"], 0.65, c["min_gt_h"])
    rois, r3, cen = grids_of(c, dev)
    d = {k: _t(gt[k], dev) for k in ("gts_val", "box_lbls", "gts_ign", "gts_3d", "val_counts", "ign_counts")}
    p2, scale = _t(c["p2"], dev), _t(c["scale_factor"], dev)
    means, stds = c["means"], c["stds"]
    t = targets.compute_targets_batched(rois, d["gts_val"], d["box_lbls"], conf.fg_thresh, 0.5, 0.0, 0.5, 0.35, gts_ign=d["gts_ign"],
                                        val_counts=d["val_counts"], ign_counts=d["ign_counts"], gts_3d=d["gts_3d"], rois_3d=r3, rois_3d_cen=cen,
                                        anchor_cols=c["anchors"].shape[1], means=means, stds=stds, want=("transforms", "raw_gt"))
    s = sampling.sample_anchors(t.transforms[..., 4], x["prob"], d["val_counts"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])
    l_cls, _ = sampling.classification_loss(x["cls"], s, fg_fraction=c["fg_fraction"], focal_loss=c["focal_loss"], cls_2d_lambda=1)
    acc = x["acceptance"][:, :, 0] if x["acceptance"] is not None else None
    l_nms, _ = after_nms.after_nms_loss(x["prob"], acc, x["bbox_2d"], x["bbox_3d"], t, s, rois, r3, cen, p2, scale, d["gts_val"], d["gts_3d"],
                                        d["val_counts"], means=means, stds=stds, after_nms_lambda=0.05,
                                        after_nms_loss_mode="classify" if c["mode"] == "classify" else "rank",
                                        rank_boxes_of_all_images_at_once=c["mode"] == "rank_all", temperature=0.1)
    l_reg, st = regression.regression_loss(x["bbox_2d"], x["bbox_3d"], acc, t, s, rois, r3, cen, p2, scale, means=means, stds=stds,
                                           bbox_2d_lambda=c["bbox_2d_lambda"], bbox_3d_lambda=1, bbox_axis_head_lambda=0.35, iou_2d_lambda=1,
                                           use_acceptance_prob_in_regression_loss=acc is not None, bbox_un_dynamic=acc is not None,
                                           un_state=regression.new_un_state(dev) if acc is not None else None)
    return l_cls + l_nms + l_reg, st


@pytest.mark.parametrize("cid", ["r210/reference", "r210/classify", "r210/no_acceptance", "r210/mixed", "cap/cap"])
def test_gradients_equal_the_hand_composition_bit_for_bit(dev, cid):
    """cls + after-NMS + regression through their own Functions and autograd's sum, against the module's one backward launch (g = 1)"""
    c = H.case_of(cid)
    g, _ = run_module(dev, c)
    x = leaves_of(c, dev)
    loss, st = hand_composition(dev, c, x)
    loss.backward()
    torch.cuda.synchronize()
    for k in HEADS:
        if x[k] is None:
            continue
        mine = x[k].grad.cpu().numpy().reshape(c[k].shape) if x[k].grad is not None else np.zeros(c[k].shape, np.float32)
        assert np.array_equal(g["grad_" + k], mine), (cid, k)
    assert g["grad_cls"].any() and g["grad_bbox_3d"].any() and g["grad_bbox_2d"].any()
    assert abs(g["total"] - float(loss.detach().cpu())) <= 4 * H.ulp32(g["total"])
    for k in ("bbox_3d", "un", "iou_2d_los", "z", "rot", "cen", "iou_2d"):
        if k in g["stats"]:
            assert g["stats"][k] == float(st[k].cpu()), k


@pytest.mark.parametrize("cid", ["r210/reference", "r210/no_acceptance"])
def test_backward_launch_scales_by_the_upstream_gradient(dev, cid):
    """loss.backward(); (3 * loss).backward(); torch.autograd.grad with a device scalar: g x the unit gradients to 1 ulp.  With an
    acceptance head no term reads prob (its gradient is zeros); without one the scores do, and the acceptance part is absent"""
    c = H.case_of(cid)
    unit, _ = run_module(dev, c)
    three, _ = run_module(dev, c, upstream=3.0)
    scalar = torch.tensor(0.37, device=dev)
    frac, _ = run_module(dev, c, backward="grad", upstream=scalar)
    for k in H.GRADS:
        if k == "grad_acceptance" and not c["has_acceptance"]:
            assert unit[k] is None and three[k] is None and frac[k] is None
            continue
        assert bool(unit[k].any()) == (k != "grad_prob" or not c["has_acceptance"]), k
        for got, s in ((three[k], np.float32(3.0)), (frac[k], np.float32(0.37))):
            want = unit[k] * s
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (k, float(s))
    assert three["total"] == unit["total"] == frac["total"]


def test_backward_launch_optional_parts_and_widths(dev):
    """prob without a gradient; bbox_3d with 10 and with 11 columns; B = 1 (R = 210 is no multiple of 64 or of the vector width)"""
    c = H.case_of("r210/reference")
    full, _ = run_module(dev, c)
    part, _ = run_module(dev, c, no_grad=("prob",))
    assert part["grad_prob"] is None and full["grad_prob"] is not None
    for k in ("grad_cls", "grad_bbox_2d", "grad_bbox_3d", "grad_acceptance"):
        assert np.array_equal(part[k], full[k]), k
    ten = dict(c, bbox_3d=np.ascontiguousarray(c["bbox_3d"][:, :, :10]))
    g10, _ = run_module(dev, ten)
    assert g10["grad_bbox_3d"].shape == (2, 210, 10) and full["grad_bbox_3d"].shape == (2, 210, 11)
    assert np.array_equal(g10["grad_bbox_3d"], full["grad_bbox_3d"][:, :, :10]) and not full["grad_bbox_3d"][:, :, 10].any()
    assert g10["total"] == full["total"] and np.array_equal(g10["grad_cls"], full["grad_cls"])
    # B = 1: image 0 alone; the per-anchor arithmetic is the parent case's, whose e is the scale of fp32 against float64 here too
    one = one_image(c)
    g1, _ = run_module(dev, one)
    assert g1["grad_cls"].shape == (1, 210, 4)
    check_against(g1, H.restate_loss(one), H.stored_errors("r210/reference"), "r210/reference image 0", 4)


def test_anchor_grid_when_the_tables_are_absent(dev):
    """rois / rois_3d / rois_3d_cen left out: heads.anchor_grid(conf.anchors, feat_size, conf.feat_stride), the same bits as passing them"""
    from groomed_nms_amd import heads
    from groomed_nms_amd.loss import RPN_3D_loss
    c = H.case_of("r210/reference")
    outs = []
    for explicit in (False, True):
        m = RPN_3D_loss(H.conf_of(c))
        x = leaves_of(c, dev)
        kw = {}
        if explicit:
            kw = dict(zip(("rois", "rois_3d", "rois_3d_cen"), heads.anchor_grid(c["anchors"], (5, 7), 16, batch=2, device=dev)))
        loss, _ = m(x["cls"], x["prob"], x["bbox_2d"], x["bbox_3d"], imobjs_of(c), [5, 7], bbox_acceptance_prob=x["acceptance"], **kw)
        loss.backward()
        outs.append((loss.detach().clone(), m.last_stats.clone(), x["cls"].grad.clone(), x["bbox_3d"].grad.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert torch.isfinite(outs[0][0])


def test_graph_capture_forward_packed_and_backward(dev):
    """forward_packed + loss.backward() captured once on static buffers (a host read inside would fail the capture); replayed after the
    records and heads were overwritten with a second scene -- other counts, an image without a valid ground truth -- it meets that
    scene's restatement by the rule; two consecutive replays advance the uncertainty state as two eager calls do"""
    from groomed_nms_amd.loss import RPN_3D_loss, pack_ground_truths, GroundTruths
    first, second = H.case_of("r210/mixed"), H.case_of("r210/no_gt_image")
    assert first["counts"].tolist() != second["counts"].tolist() and H.restated("r210/no_gt_image")["gt"]["val_counts"][1] == 0
    m = RPN_3D_loss(H.conf_of(second))
    rng = np.random.default_rng(9)
    data = {k: _t(first[k] * np.float32(rng.uniform(0.8, 0.95)), dev) for k in HEADS}      # other heads than the replay's
    data["acceptance"] = data["acceptance"].unsqueeze(2).contiguous()
    gt = GroundTruths.empty(2, H.CAPACITY, device=dev)
    pack_ground_truths(imobjs_of(first), H.LBLS, H.ILBLS, capacity=H.CAPACITY).to(dev, out=gt)
    rois, r3, cen = grids_of(second, dev)

    def step(mod):
        # (leaves of the step's own: one kept across steps carries a gradient accumulator bound to the stream of its first use)
        x = {k: data[k].detach().requires_grad_(True) for k in HEADS}
        loss, _ = mod.forward_packed(x["cls"], x["prob"], x["bbox_2d"], x["bbox_3d"], gt, rois, r3, cen, x["acceptance"])
        loss.backward()
        return [loss.detach(), mod.last_stats] + [x[k].grad for k in HEADS]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(m)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state = m.un_state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(m)
    assert m.un_state is state
    # the second scene into the same buffers
    with torch.no_grad():
        for k in HEADS:
            data[k].copy_(_t(second[k], dev).reshape(data[k].shape))
        state.copy_(torch.zeros(2, dtype=torch.float64))
    pack_ground_truths(imobjs_of(second), H.LBLS, H.ILBLS, capacity=H.CAPACITY).to(dev, out=gt)
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in out]
    g = {"total": float(got[0].cpu()), "stats": {key: float(got[1][H.STAT_KEYS.index(key)].cpu()) for _, key in m.stat_entries()}}
    for k, v in zip(HEADS, got[2:]):
        g["grad_" + k] = v.cpu().numpy().reshape(second[k].shape)
    check_against(g, H.restated("r210/no_gt_image"), H.stored_errors("r210/no_gt_image"), "replayed r210/no_gt_image", 4)
    graph.replay()
    torch.cuda.synchronize()
    twice = [o.clone() for o in out]
    state_replayed = state.clone()
    eager = RPN_3D_loss(H.conf_of(second))
    e1 = [o.clone() for o in step(eager)]
    e2 = [o.clone() for o in step(eager)]
    torch.cuda.synchronize()
    assert torch.equal(state_replayed, eager.un_state) and float(state_replayed[0]) == 2.0
    for a, b in zip(got + twice, e1 + e2):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
