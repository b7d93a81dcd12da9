"""CPU-side tests of the anchor sampler and the weighted classification term (groomed_nms_amd/sampling.py, csrc/sampling.hip).

`restate` below is the checker: a NumPy / float64 restatement of what lib/loss/rpn_3d.py does between compute_targets and the
classification term, with the line numbers of the reference.  It is checked here against tests/golden/sampling.npz (the reference's own
RPN_3D_loss.forward, tests/golden/make_sampling_golden.py); the GPU tests (test_sampling_gpu.py) then check the kernels against it and
take from here, per golden case, e_ref = |reference - restatement| of the loss and of the gradient.
Ties at a quota: np.argsort's order among equal keys is not defined; the project's rule, and the checker's, is lowest anchor index first.
"""
import ast
import ctypes
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampling.npz")

IGN_FLAG = 3000            # lib/loss/rpn_3d.py:184
EPS32 = 2.0 ** -24         # half an ulp of a float32 in [1, 2): one rounding


def restate(target_labels, prob, val_counts, cls=None, *, box_samples, fg_fraction, focal_loss=0, cls_2d_lambda=1):
    """target_labels [B, R], prob [B, R, C] float32, val_counts [B] (0: the image has no valid GT), cls [B, R, C] float32 or None.
    Returns a dict: labels, enc (0 / 1 fg / 2 bg), bbox_weights, labels_scores, counts [B, 6], fg_lists, and with cls: labels_weight
    (float32), loss (float64), grad (float64), acc_fg, acc_bg, n_active."""
    prob = np.asarray(prob)
    t_all = np.asarray(target_labels)
    B, R, C = prob.shape
    labels = np.zeros((B, R))                                                # :300-303
    enc = np.zeros((B, R), np.int64)
    labels_scores = np.zeros((B, R))
    bbox_weights = np.zeros((B, R))
    counts = np.zeros((B, 6), np.int64)
    fg_lists = []
    for b in range(B):
        if val_counts is not None and val_counts[b] <= 0:                    # :406 `continue`: nothing below runs for the image
            fg_lists.append(np.zeros(0, np.int64))
            continue
        t = t_all[b]
        fg_inds = np.flatnonzero(t > 0)                                      # :459-465
        bg_inds = np.flatnonzero(t < 0)
        ign_inds = np.flatnonzero(t == 0)
        labels[b, fg_inds] = t[fg_inds]                                      # :470-472
        labels[b, ign_inds] = IGN_FLAG
        labels[b, bg_inds] = 0
        n_fg, n_bg = len(fg_inds), len(bg_inds)
        if box_samples == np.inf:                                            # :583-588
            fg_num, bg_num = n_fg, n_bg
        else:
            fg_num = min(round(R * box_samples * fg_fraction), n_fg)
            bg_num = min(round(R * box_samples - fg_num), n_bg)
        if fg_num > 0 and fg_num != n_fg:                                    # :591-595 (stable: ties lowest index first; NaN last)
            scores = prob[b, fg_inds, labels[b, fg_inds].astype(int)]
            fg_inds = fg_inds[np.argsort(scores, kind="stable")][:fg_num]
        if bg_num > 0 and bg_num != n_bg:                                    # :597-601
            scores = prob[b, bg_inds, labels[b, bg_inds].astype(int)]
            bg_inds = bg_inds[np.argsort(scores, kind="stable")][:bg_num]
        enc[b, bg_inds] = 2                                                  # :610-612
        enc[b, fg_inds] = 1
        bbox_weights[b, fg_inds] = 1
        active = labels[b] != IGN_FLAG                                       # :886-887
        labels_scores[b, active] = prob[b, active, labels[b, active].astype(int)]
        counts[b] = (n_fg, n_bg, fg_num, bg_num, len(fg_inds), len(bg_inds))
        fg_lists.append(np.sort(fg_inds))
    out = dict(labels=labels.astype(np.int64), enc=enc, bbox_weights=bbox_weights.astype(np.float32),
               labels_scores=labels_scores.astype(np.float32), counts=counts, fg_lists=fg_lists)
    if cls is None:
        return out
    x = np.asarray(cls).astype(np.float64)
    cls_pred = np.argmax(np.asarray(cls), axis=2)                            # :899
    fg_all = (labels > 0) & (labels != IGN_FLAG)                             # :893-894
    bg_all = (labels == 0) & (labels != IGN_FLAG)
    out["acc_fg"] = np.mean(cls_pred[fg_all] == labels[fg_all]) if fg_all.any() else np.nan       # :901-907
    out["acc_bg"] = np.mean(cls_pred[bg_all] == labels[bg_all]) if bg_all.any() else np.nan
    out["stat_counts"] = (int((cls_pred[fg_all] == labels[fg_all]).sum()), int(fg_all.sum()),
                          int((cls_pred[bg_all] == labels[bg_all]).sum()), int(bg_all.sum()))
    fg = enc == 1                                                            # :913-918
    bg = enc == 2
    fg_num, bg_num = int(fg.sum()), int(bg.sum())
    w = np.zeros((B, R))                                                     # :920-938
    w[fg | bg] = 1.0
    if fg_fraction is not None and fg_num > 0:
        w[fg] = (fg_fraction / (1 - fg_fraction)) * (bg_num / fg_num)
    if focal_loss:                                                           # :945-961
        if bg_num > 0:
            w[bg] *= (1 - labels_scores[bg]) ** focal_loss
        if fg_num > 0:
            w[fg] *= (1 - labels_scores[fg]) ** focal_loss
    w32 = w.astype(np.float32)                                               # :970-971
    out["labels_weight"] = w32
    out["labels_weight_f64"] = w
    act = w32 > 0                                                            # :979
    n = int(act.sum())
    out["n_active"] = n
    grad = np.zeros((B, R, C))
    loss = 0.0
    if cls_2d_lambda and n > 0:                                              # :976-1001, in float64
        xa = x[act]
        la = labels[act].astype(int)
        m = xa.max(axis=1, keepdims=True)
        lse = np.log(np.exp(xa - m).sum(axis=1, keepdims=True))
        lsm = xa - m - lse
        ce = -lsm[np.arange(n), la]
        wl = ce * w32[act].astype(np.float64)
        inside = (wl >= 0) & (wl <= 2000)
        loss = float(np.clip(wl, 0, 2000).mean() * cls_2d_lambda)
        onehot = np.zeros_like(xa)
        onehot[np.arange(n), la] = 1.0
        g = (cls_2d_lambda / n) * w32[act].astype(np.float64)[:, None] * (np.exp(lsm) - onehot)
        g[~inside] = 0.0
        grad[act] = g
    out["loss"] = loss
    out["grad"] = grad
    return out


# ---------------------------------------------------------------------------------------------- the goldens

@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        parts = key.split("/")
        if len(parts) == 3:
            cases.setdefault((parts[0], parts[1]), {})[parts[2]] = z[key]
    for (shape, _), c in cases.items():
        c["cls"] = z[shape + "/cls"]
        c["prob"] = z[shape + "/prob"]
        bs, ff, focal = c["config"]
        c["box_samples"] = float(bs)
        c["fg_fraction"] = None if np.isnan(ff) else float(ff)
        c["focal_loss"] = int(focal)
    return cases


def case_ids():
    return sorted("%s/%s" % k for k in golden())


def case_of(cid):
    return golden()[tuple(cid.split("/"))]


@functools.lru_cache(maxsize=None)
def restated(cid):
    c = case_of(cid)
    return restate(c["target_labels"], c["prob"], c["val_counts"], c["cls"], box_samples=c["box_samples"],
                   fg_fraction=c["fg_fraction"], focal_loss=c["focal_loss"], cls_2d_lambda=1)


@functools.lru_cache(maxsize=None)
def reference_errors(cid):
    """e_ref of a golden case: |reference - float64 restatement| of the loss, and the largest such difference over the gradient"""
    c, r = case_of(cid), restated(cid)
    return abs(float(c["loss"]) - r["loss"]), float(np.abs(c["grad"].astype(np.float64) - r["grad"]).max())


def test_golden_holds_the_cases_of_both_shapes():
    names = {"both_cut", "both_cut_focal2", "neither", "neither_focal2", "bg_cut", "quota_zero", "inf", "inf_no_fraction",
             "inf_no_fraction_focal2", "no_gt_image", "all_ignored_image"}
    assert {k for k in golden()} == {(s, n) for s in ("r210", "r1332") for n in names}
    assert case_of("r210/both_cut")["prob"].shape == (2, 210, 4) and case_of("r1332/both_cut")["prob"].shape == (2, 1332, 4)
    assert os.path.getsize(GOLDEN) < 1 << 20
    # the regimes the cases are there for
    r = restated("r210/both_cut")["counts"]
    assert (r[:, 2] < r[:, 0]).all() and (r[:, 3] < r[:, 1]).all() and (r[:, 2] > 0).all()
    assert r[0, 3] == 50                                   # round(210 * 0.25 - 2) = round(50.5) = 50: half to even
    r = restated("r1332/quota_zero")["counts"]
    assert (r[:, 2:4] == 0).all() and (r[:, 4] == r[:, 0]).all() and (r[:, 5] == r[:, 1]).all()     # a quota of 0 cuts nothing
    r = restated("r1332/bg_cut")["counts"]
    assert (r[:, 4] == r[:, 0]).all() and (r[:, 5] < r[:, 1]).all()
    assert restated("r210/no_gt_image")["counts"][1].sum() == 0 and restated("r210/all_ignored_image")["counts"][0].sum() == 0
    for cid in case_ids():
        assert (restated(cid)["labels"] == IGN_FLAG).any(), cid


@pytest.mark.parametrize("cid", case_ids())
def test_restatement_matches_the_reference(cid):
    c, r = case_of(cid), restated(cid)
    # the reference's gradient on cls is non-zero exactly on the sampled anchors
    sampled_ref = (c["grad"] != 0).any(axis=2)
    assert np.array_equal(sampled_ref, r["enc"] != 0), "sampled set differs from the reference's"
    assert np.array_equal(sampled_ref, r["labels_weight"] > 0)
    fg_ref, bg_ref, cls_ref = c["stats"]
    assert fg_ref == r["acc_fg"] and bg_ref == r["acc_bg"]
    # float32 rounding.  Loss: a float32 chain of <= 8 roundings per anchor (x - m, exp, the sum over C = 4, log, two subtractions, the
    # weight) and <= 12 more in the float32 mean, each relative to terms up to ~3x the result (lse - (x_l - m) cancels): 64 roundings
    e_loss, e_grad = reference_errors(cid)
    print("%s: e_ref loss %.3e (%.2f float32 roundings of the loss), grad %.3e (%.2f of its largest entry)"
          % (cid, e_loss, e_loss / (EPS32 * abs(r["loss"])), e_grad, e_grad / (EPS32 * np.abs(r["grad"]).max())))
    assert e_loss <= 64 * EPS32 * abs(r["loss"])
    assert abs(float(cls_ref) - r["loss"]) <= 64 * EPS32 * abs(r["loss"])
    # Gradient: exp of a float32 log-softmax whose absolute rounding error is ~ |x - m| <= ~12 roundings, then three products
    assert e_grad <= 32 * EPS32 * np.abs(r["grad"]).max()
    # and each entry is proportional to its anchor's weight: the rows sum to zero up to rounding
    assert np.abs(c["grad"].sum(axis=2)).max() <= 32 * EPS32 * np.abs(r["grad"]).max()


def test_restatement_tie_rule_and_nan_last():
    """among equal keys the lower index first; NaN keys last (np.argsort)"""
    R = 12
    t = -np.ones((1, R), np.float32)
    t[0, [1, 7]] = 2
    prob = np.full((1, R, 4), 0.25, np.float32)
    prob[0, 3, 0] = np.nan
    prob[0, 9, 0] = 0.125
    r = restate(t, prob, np.array([1]), box_samples=0.5, fg_fraction=0.5)          # fg quota 3 >= 2: no cut; bg quota round(6 - 2) = 4 of 10
    assert r["counts"][0].tolist() == [2, 10, 2, 4, 2, 4]
    assert np.flatnonzero(r["enc"][0] == 2).tolist() == [0, 2, 4, 9]
    assert r["fg_lists"][0].tolist() == [1, 7]
    prob[0, :, 0] = np.nan
    prob[0, 11, 0] = 0.5
    r = restate(t, prob, np.array([1]), box_samples=0.5, fg_fraction=0.5)
    assert np.flatnonzero(r["enc"][0] == 2).tolist() == [0, 2, 3, 11]


# ---------------------------------------------------------------------------------------------- ABI and module

NEW_SYMBOLS = ("gnms_sample_anchors_workspace_bytes", "gnms_sample_anchors", "gnms_cls_loss_workspace_bytes", "gnms_cls_loss")


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    words = decl.replace("const", " ").split()[:-1]          # drop the parameter's name
    return {"int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "double": ctypes.c_double, "float": ctypes.c_float,
            "int": ctypes.c_int}[" ".join(words)]


def test_abi_symbols_and_prototypes(lib):
    from groomed_nms_amd import _lib
    text = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^;{}]*)\)\s*;" % name, text)
        assert m, "%s is not declared in the header" % name
        res = {"size_t": ctypes.c_size_t, "int": ctypes.c_int}[m.group(1)]
        args = [_ctype_of(a) for a in m.group(2).split(",")]
        assert _lib._SIGNATURES[name] == (res, args), "%s: the ctypes prototype and the header disagree" % name
    assert lib.gnms_abi_version() == 1


def test_argument_errors_without_gpu(lib):
    """every check below returns before a HIP call"""
    fake = ctypes.c_void_p(1 << 20)
    INVALID, WORKSPACE = -1, -4            # GNMS_ERR_INVALID_ARGUMENT, GNMS_ERR_WORKSPACE
    outs = [fake] * 7
    rc = lib.gnms_sample_anchors(fake, 1, fake, None, 2, 64, 1, 0.2, 1, 0.2, *outs, fake, 1 << 30, None)
    assert rc == INVALID and b"C = 1" in lib.gnms_last_error()
    assert lib.gnms_sample_anchors(fake, 1, fake, None, 2, 0, 4, 0.2, 1, 0.2, *outs, fake, 1 << 30, None) == INVALID
    for k in range(7):
        o = list(outs)
        o[k] = None
        assert lib.gnms_sample_anchors(fake, 1, fake, None, 2, 64, 4, 0.2, 1, 0.2, *o, fake, 1 << 30, None) == INVALID
        assert b"NULL" in lib.gnms_last_error()
    assert lib.gnms_sample_anchors(fake, 1, fake, None, 2, 64, 4, 0.2, 0, 0.0, *outs, fake, 1 << 30, None) == INVALID   # finite, no fraction
    assert lib.gnms_sample_anchors(fake, 1, fake, None, 2, 64, 4, -1.0, 1, 0.2, *outs, fake, 1 << 30, None) == INVALID
    need = lib.gnms_sample_anchors_workspace_bytes(2, 126720)
    assert 0 < need < 4 << 20 and lib.gnms_sample_anchors_workspace_bytes(0, 5) == 0
    assert lib.gnms_sample_anchors(fake, 1, fake, None, 2, 126720, 4, 0.2, 1, 0.2, *outs, fake, need - 1, None) == WORKSPACE
    assert b"workspace" in lib.gnms_last_error()
    co = [fake] * 5
    ins = [fake] * 5
    assert lib.gnms_cls_loss(*ins, 2, 64, 1, 1, 0.2, 0.0, 1.0, *co, fake, 1 << 30, None) == INVALID
    assert lib.gnms_cls_loss(*ins, 2, 0, 4, 1, 0.2, 0.0, 1.0, *co, fake, 1 << 30, None) == INVALID
    for k in range(5):
        o = list(co)
        o[k] = None
        assert lib.gnms_cls_loss(*ins, 2, 64, 4, 1, 0.2, 0.0, 1.0, *o, fake, 1 << 30, None) == INVALID
    need = lib.gnms_cls_loss_workspace_bytes(2, 126720)
    assert need > 0
    assert lib.gnms_cls_loss(*ins, 2, 126720, 4, 1, 0.2, 0.0, 1.0, *co, fake, need - 1, None) == WORKSPACE


def test_module_surface():
    import groomed_nms_amd
    from groomed_nms_amd import sampling
    assert "sample_anchors" in sampling.__all__ and "classification_loss" in sampling.__all__
    assert groomed_nms_amd.sample_anchors is sampling.sample_anchors
    assert groomed_nms_amd.classification_loss is sampling.classification_loss
    assert sampling.Sample._fields == ("labels", "labels_scores", "bbox_weights", "fg_index", "fg_counts", "counts")
    assert sampling.IGN_FLAG == IGN_FLAG
    with pytest.raises(NotImplementedError):
        sampling.sample_anchors(None, None, None, box_samples=0.2, fg_fraction=0.2, hard_negatives=False)


def test_product_does_not_import_the_checker():
    src = open(os.path.join(ROOT, "groomed_nms_amd", "sampling.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            mods.add((node.module or "").split(".")[0])
    assert not mods & {"oracle", "tests", "test_sampling_host", "numpy"}, mods
