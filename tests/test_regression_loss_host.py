"""CPU-side tests of the box regression, 2D IoU and uncertainty terms of the RPN loss (groomed_nms_amd/regression.py, csrc/regression.hip).

`restate` below is the checker: a NumPy / float64 restatement of what lib/loss/rpn_3d.py does with the sampled foreground (:1154-1407,
fed by :206-233, :316-363, :477-579, :617-621), with the line numbers of the reference, and of autograd's gradients w.r.t. the three
heads, written out by hand.  It is checked here against tests/golden/regression.npz (the reference's own RPN_3D_loss.forward and
backward, tests/golden/make_regression_golden.py); the GPU tests (test_regression_loss_gpu.py) then check the kernels against it and take
from here, per golden case, e_ref = |reference - restatement| of the loss, of each statistic and of each gradient (largest entry).
The active set comes from test_sampling_host.restate (the sampler's checker).

The bounds on e_ref (u = 2^-24, one float32 rounding; the reference computes in float32, the restatement in float64):
  a mean of n terms   float32 recursive summation costs at most n u sum|term_i|, each term carries c roundings of its own (c counted
                      per group in GROUP_OPS: 2D 4, 3D 5 with the weighting, cross entropy 8, uncertainty 2, -log IoU 20 from the
                      decode to the log) and the division one more: (n + c + 1) u mean|term|, times the term's weight.
  the loss            the sum of its terms' bounds, plus COMBINE_OPS = 16 roundings of the partial sums (nine means added, two
                      products with the weights, four `loss +=`, one for `total`), each at most u times the sum of the terms' magnitudes.
  the running weight  this step's init is nine unweighted means combined in nine operations and enters the weight with 1 / n_frames:
                      (n + 8 + 1 + 9) u (sum of the means' magnitudes) / n_frames.
  a statistic         (n + c + 1) u mean|term| with c: cen 24 (three decodes of 6, three squares, two sums, the root), z 7, rot 8,
                      iou_2d 20, conf 0; the counts' ratios (axis, head, cen_dist_lt_0.2) are exact up to one division.
  a gradient entry    K_GRAD u |largest entry|, K_GRAD = 32 float32 operations on the longest path, bbox_2d's through the IoU:
                      forward dx std, + mean, times width, + centre (4), exp, times width, halved (7), the corner's difference, - 1
                      (9), the overlap's difference (10), the product of the overlaps (11), the areas (13), the union's sum and
                      difference (15), the quotient (16), log (17), the mean's division (18); backward 1 / n, -1 / iou, 1 / union,
                      inter / union^2, the two sums into the corner's gradient, times the other overlap, the halves, times exp, times
                      width, times std, the sum of the two corners (32).  bbox_3d's and acceptance's paths are shorter (<= 12).
Measured: the largest e_ref is 0.97 of its bound (the bbox_2d gradient of r1332/inf), every other at most 0.38.
"""
import ast
import ctypes
import functools
import os
import re

import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling_host import restate as restate_sampling  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "regression.npz")
EPS32 = 2.0 ** -24
STAT_NAMES = ["bbox_2d", "bbox_3d", "un", "iou_2d_los", "cen", "cen_dist_lt_0.2", "z", "rot", "iou_2d", "axis", "head", "conf", "total"]
GROUP_OPS = {"2d": 4, "3d": 5, "bce": 8, "un": 2, "iou": 20}
COMBINE_OPS = 16
K_GRAD = 32
SNAP_TRIPS = 1024


def smooth_l1(x, t):
    d = x - t
    z = np.abs(d)
    return np.where(z < 1.0, 0.5 * z * z, z - 0.5), np.where(d <= -1.0, -1.0, np.where(d >= 1.0, 1.0, d))


def bce(p, y):
    """F.binary_cross_entropy: the logs clamped at -100; its backward's denominator clamped at 1e-12"""
    with np.errstate(all="ignore"):
        lp = np.log(p)
        lq = np.log1p(-p)
    lp = np.where(lp < -100.0, -100.0, lp)
    lq = np.where(lq < -100.0, -100.0, lq)
    den = (1.0 - p) * p
    with np.errstate(all="ignore"):
        return (y - 1.0) * lq - y * lp, (p - y) / np.where(den > 1e-12, den, 1e-12)


def snap_to_pi(a):
    a = a.copy()
    fin = np.isfinite(a)
    for _ in range(SNAP_TRIPS):
        m = fin & (a > np.pi)
        if not m.any():
            break
        a[m] -= 2 * np.pi
    for _ in range(SNAP_TRIPS):
        m = fin & (a <= -np.pi)
        if not m.any():
            break
        a[m] += 2 * np.pi
    return a


def decode_2d(d, means, stds, w, h, cx, cy):
    """bbox_transform_inv, rpn_util.py:886-934"""
    dx, dy, dw, dh = (d[:, k] * stds[k] + means[k] for k in range(4))
    px, py = dx * w + cx, dy * h + cy
    with np.errstate(all="ignore"):
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
    return np.stack([px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw - 1.0, py + 0.5 * ph - 1.0], 1), pw, ph


def _mean(s, c):
    return s / c if c else np.nan


def restate(bbox_2d, bbox_3d, acceptance, transforms, raw_gt, rois, rois_3d, rois_3d_cen, p2, scale_factor, fg_lists, fg_num, *, means, stds,
            bbox_2d_lambda, bbox_3d_lambda, bbox_axis_head_lambda, iou_2d_lambda, use_acceptance, bbox_un_lambda, bbox_un_dynamic,
            state_in=(0.0, 0.0)):
    """All arrays as regression_loss takes them (float32 data, any float dtype), fg_lists: per image the active anchors in ascending
    order, fg_num [B]: the reference's quota (Sample.counts[:, 2]).  Returns a dict: loss, stats (dict), grad_bbox_2d, grad_bbox_3d,
    grad_acceptance (float64), n, weighted, has_iou, state_out, finite counts, and mean_abs: the terms' magnitudes that the e_ref bounds need."""
    f = lambda x: np.asarray(x, np.float64)      # noqa: E731
    B, R = bbox_2d.shape[:2]
    D3 = bbox_3d.shape[2]
    means, stds = f(means), f(stds)
    bi = np.concatenate([np.full(len(l), b, np.int64) for b, l in enumerate(fg_lists)]) if B else np.zeros(0, np.int64)
    ri = np.concatenate([np.asarray(l, np.int64) for l in fg_lists]) if B else np.zeros(0, np.int64)
    n = len(ri)                                                                    # :1154-1158
    nf, W = float(state_in[0]), float(state_in[1]) if bbox_un_dynamic else float(bbox_un_lambda)
    out = dict(n=n, grad_bbox_2d=np.zeros((B, R, 4)), grad_bbox_3d=np.zeros((B, R, D3)), grad_acceptance=np.zeros((B, R)),
               weighted=bool(use_acceptance), has_iou=False, state_out=(nf, W), active=(bi, ri))
    if n == 0:
        out["loss"] = 0.0
        out["stats"] = dict({k: np.nan for k in STAT_NAMES}, bbox_un_lambda=W)
        return out
    b2, b3, tr, gt = f(bbox_2d[bi, ri]), f(bbox_3d[bi, ri]), f(transforms[bi, ri]), f(raw_gt[bi, ri])
    roi, r3, cen = f(rois[bi, ri]), f(rois_3d[bi, ri]), f(rois_3d_cen[bi, ri])
    acc = f(acceptance[bi, ri]) if acceptance is not None else np.ones(n)
    P = f(p2)[bi]
    sc = f(scale_factor)[bi]
    stats, mean_abs = {}, {}

    # ---- 2D term, :1163-1191 (the prediction as the network gave it)
    s2d, g2d = smooth_l1(b2, tr[:, :4])
    t2d = 0.0
    if bbox_2d_lambda:
        t2d = sum(s2d[:, k].sum() / n for k in range(4)) * bbox_2d_lambda
        mean_abs["2d"] = bbox_2d_lambda * np.abs(s2d).sum() / n
    # ---- 3D elements, :1232-1238, :1273-1287
    use_sin = gt[:, 19] == 1.0
    s3 = np.zeros((n, 7))
    g3 = np.zeros((n, 7))
    s3[:, :6], g3[:, :6] = smooth_l1(b3[:, :6], tr[:, 5:11])
    s3[:, 6], g3[:, 6] = smooth_l1(np.where(use_sin, b3[:, 6], b3[:, 7]), np.where(use_sin, tr[:, 12], tr[:, 13]))
    ce = np.zeros((n, 2))
    gce = np.zeros((n, 2))
    ce[:, 0], gce[:, 0] = bce(b3[:, 8], gt[:, 19])
    ce[:, 1], gce[:, 1] = bce(b3[:, 9], gt[:, 20])
    # ---- decode and statistics, :318-357, :532-577, :1194-1209
    w = roi[:, 2] - roi[:, 0] + 1.0
    h = roi[:, 3] - roi[:, 1] + 1.0
    x_dn = (b3[:, 0] * stds[4] + means[4]) * w + cen[:, 0]
    y_dn = (b3[:, 1] * stds[5] + means[5]) * h + cen[:, 1]
    z_dn = r3[:, 4] + (b3[:, 2] * stds[6] + means[6])
    z_raw = z_dn - P[:, 2, 3]                                                       # :553-555
    x_raw = ((z_raw + P[:, 2, 3]) * (x_dn / sc) - P[:, 0, 2] * z_raw - P[:, 0, 3]) / P[:, 0, 0]
    y_raw = ((z_raw + P[:, 2, 3]) * (y_dn / sc) - P[:, 1, 2] * z_raw - P[:, 1, 3]) / P[:, 1, 1]
    cen_dist = np.sqrt((x_raw - gt[:, 12]) ** 2 + (y_raw - gt[:, 13]) ** 2 + (z_raw - gt[:, 14]) ** 2)      # :1202-1204
    stats["cen"] = cen_dist.mean()
    stats["cen_dist_lt_0.2"] = (cen_dist <= 0.2).mean()                             # :1206
    stats["z"] = np.abs(z_raw - gt[:, 14]).mean()                                   # :576, :1385
    rot = np.where(use_sin, r3[:, 9] + (b3[:, 6] * stds[11] + means[11]), r3[:, 10] + (b3[:, 7] * stds[12] + means[12]))    # :327-328, :362-363, :569-570
    rot = rot + np.where(gt[:, 20] == 1.0, np.pi, 0.0)                              # :571
    stats["rot"] = np.abs(snap_to_pi(rot) - gt[:, 11]).mean()                       # :573, :577, :1388
    mean_abs["cen"], mean_abs["z"], mean_abs["rot"] = stats["cen"], stats["z"], stats["rot"]

    # ---- 3D term, :1299-1373
    t3d = 0.0
    cnt_u = np.isfinite(s3).sum(0)
    cnt_ce = np.isfinite(ce).sum(0)
    out["finite_unweighted"] = [int(c) for c in cnt_u] + [int(c) for c in cnt_ce]
    weighted = bool(use_acceptance)
    write_state = False
    stats["axis"] = stats["head"] = np.nan
    stats["conf"] = acc.mean() if acceptance is not None and bbox_3d_lambda else np.nan      # :1355-1356, inside `if self.bbox_3d_lambda`
    c3 = np.zeros(7)
    cah = 0.0
    wgt = np.ones(n)
    fin_w = np.isfinite(s3)
    if bbox_3d_lambda:
        stats["axis"] = (np.where(b3[:, 8] >= 0.5, 1.0, 0.0) == gt[:, 19]).mean()   # :1292
        stats["head"] = (np.where(b3[:, 9] >= 0.5, 1.0, 0.0) == gt[:, 20]).mean()   # :1297
        if bbox_un_dynamic:                                                        # :1323-1341, in the order w, h, l, rot, x, y, z
            init = sum(_mean(np.where(np.isfinite(s3[:, k]), s3[:, k], 0.0).sum(), cnt_u[k]) for k in (3, 4, 5, 6, 0, 1, 2)) * bbox_3d_lambda
            init += (_mean(np.where(np.isfinite(ce[:, 0]), ce[:, 0], 0.0).sum(), cnt_ce[0])
                     + _mean(np.where(np.isfinite(ce[:, 1]), ce[:, 1], 0.0).sum(), cnt_ce[1])) * bbox_axis_head_lambda
            mean_abs["init"] = (bbox_3d_lambda * sum(_mean(np.abs(np.where(np.isfinite(s3[:, k]), s3[:, k], 0.0)).sum(), cnt_u[k]) for k in range(7))
                                + bbox_axis_head_lambda * sum(_mean(np.abs(np.where(np.isfinite(ce[:, k]), ce[:, k], 0.0)).sum(), cnt_ce[k]) for k in range(2)))
            if nf == 0:
                W, nf = init, 1.0
            else:
                nf = min(100.0, nf + 1.0)
                W = init / nf + W * (nf - 1.0) / nf
            write_state = True
            if W > 0:                                                              # :1344
                weighted = True
        if acceptance is None:
            weighted = False
        if weighted:
            wgt = acc
        e3 = s3 * wgt[:, None]                                                     # :1345-1351
        ew = ce * wgt[:, None]                                                     # :1353-1354
        fin_w = np.isfinite(e3)
        cnt_w = fin_w.sum(0)
        s = sum(_mean(np.where(fin_w[:, k], e3[:, k], 0.0).sum(), cnt_w[k]) for k in range(7))            # :1358-1364
        s += (ew[:, 0].sum() / n + ew[:, 1].sum() / n) * bbox_axis_head_lambda                             # :1367 (plain means)
        t3d = s * bbox_3d_lambda                                                   # :1369
        with np.errstate(all="ignore"):
            c3 = bbox_3d_lambda / cnt_w
        cah = bbox_3d_lambda * bbox_axis_head_lambda / n
        out["finite_weighted"] = [int(c) for c in cnt_w]
        mean_abs["3d"] = bbox_3d_lambda * sum(_mean(np.abs(np.where(fin_w[:, k], e3[:, k], 0.0)).sum(), cnt_w[k]) for k in range(7))
        mean_abs["bce"] = bbox_3d_lambda * bbox_axis_head_lambda * np.abs(ew).sum() / n
    else:
        weighted = False                                                           # no term that the acceptance could weight
    # ---- uncertainty term, :1375-1382
    tun, cun = 0.0, 0.0
    if W > 0 and acceptance is not None:
        tun = (1.0 - acc).mean() * W
        cun = -W / n
        mean_abs["un"] = abs(tun)
    # ---- IoU, :617-621 with core.py:222-240, 522-529; :1390-1405
    has_q = np.asarray(fg_num)[bi] > 0
    cx, cy = roi[:, 0] + 0.5 * w, roi[:, 1] + 0.5 * h
    A, pw, ph = decode_2d(b2, means, stds, w, h, cx, cy)
    T, _, _ = decode_2d(tr[:, :4], means, stds, w, h, cx, cy)
    with np.errstate(all="ignore"):
        ixr = np.minimum(A[:, 2], T[:, 2]) - np.maximum(A[:, 0], T[:, 0])
        iyr = np.minimum(A[:, 3], T[:, 3]) - np.maximum(A[:, 1], T[:, 1])
        ix, iy = np.where(ixr < 0, 0.0, ixr), np.where(iyr < 0, 0.0, iyr)
        inter = ix * iy
        aw, ah = A[:, 2] - A[:, 0], A[:, 3] - A[:, 1]
        bw, bh = T[:, 2] - T[:, 0], T[:, 3] - T[:, 1]
        uni = aw * ah + bw * bh - inter
        iou = np.where(has_q, inter / uni, 0.0)
        di, da = (uni + inter) / (uni * uni), -inter / (uni * uni)
        mx, my = (ixr >= 0) * 1.0, (iyr >= 0) * 1.0
        tie = lambda a, b, gt_: np.where(gt_(a, b), 1.0, np.where(a == b, 0.5, 0.0))       # noqa: E731 (torch shares a tie)
        g_x1 = -di * iy * mx * tie(A[:, 0], T[:, 0], np.greater) - da * ah
        g_x2 = di * iy * mx * tie(A[:, 2], T[:, 2], np.less) + da * ah
        g_y1 = -di * ix * my * tie(A[:, 1], T[:, 1], np.greater) - da * aw
        g_y2 = di * ix * my * tie(A[:, 3], T[:, 3], np.less) + da * aw
        giou = np.stack([(g_x1 + g_x2) * w * stds[0], (g_y1 + g_y2) * h * stds[1], 0.5 * (g_x2 - g_x1) * pw * stds[2],
                         0.5 * (g_y2 - g_y1) * ph * stds[3]], 1)
        giou = np.where(has_q[:, None], giou, 0.0)
        nl = -np.log(iou)
    fin_iou = np.isfinite(iou)
    stats["iou_2d"] = _mean(iou[fin_iou].sum(), fin_iou.sum())                     # :1392
    fin_l = np.isfinite(nl)
    tiou, ciou = 0.0, 0.0
    has_iou = bool(iou_2d_lambda) and bool((iou != 0).any())                       # :1395
    if has_iou:
        tiou = _mean(nl[fin_l].sum(), fin_l.sum()) * iou_2d_lambda                 # :1396-1402
        ciou = iou_2d_lambda / fin_l.sum() if fin_l.sum() else 0.0
        mean_abs["iou"] = abs(iou_2d_lambda) * _mean(np.abs(nl[fin_l]).sum(), fin_l.sum())
    total = t2d + t3d + tun + tiou
    stats.update({"bbox_2d": t2d, "bbox_3d": t3d, "un": tun, "iou_2d_los": tiou, "total": total, "bbox_un_lambda": W})
    # ---- autograd's gradients
    g2 = np.zeros((n, 4))
    if bbox_2d_lambda:
        g2 += bbox_2d_lambda / n * g2d
    if has_iou:
        with np.errstate(all="ignore"):
            gi = np.where(fin_l, -ciou / iou, 0.0)                                  # an element the isfinite filter dropped: 0
        g2 += np.where(gi[:, None] != 0, gi[:, None] * giou, 0.0)
    out["grad_bbox_2d"][bi, ri] = g2
    gb3 = np.zeros((n, D3))
    ga = np.zeros(n) + cun
    if bbox_3d_lambda:
        ge = np.where(fin_w, c3[None] * wgt[:, None] * g3, 0.0)
        gb3[:, :6] = ge[:, :6]
        gb3[np.arange(n), np.where(use_sin, 6, 7)] = ge[:, 6]
        gb3[:, 8] = cah * wgt * gce[:, 0]
        gb3[:, 9] = cah * wgt * gce[:, 1]
        if weighted:
            ga += np.where(fin_w, c3[None] * s3, 0.0).sum(1) + cah * (ce[:, 0] + ce[:, 1])
    out["grad_bbox_3d"][bi, ri] = gb3
    if acceptance is not None:
        out["grad_acceptance"][bi, ri] = ga
    out.update(loss=total, stats=stats, weighted=weighted, has_iou=has_iou, state_out=(nf, W) if write_state else tuple(map(float, state_in)),
               mean_abs=mean_abs, finite_iou=(int(fin_iou.sum()), int((iou != 0).sum()), int(fin_l.sum())))
    return out


# ---------------------------------------------------------------------------------------------- the goldens

@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        parts = key.split("/")
        if len(parts) == 3 and not parts[1].startswith("scene_"):
            cases.setdefault((parts[0], parts[1]), {})[parts[2]] = z[key]
    for (shape, _), c in cases.items():
        for k in ("prob", "bbox_2d", "bbox_3d", "acceptance", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor"):
            c[k] = z["%s/%s" % (shape, k)]
        for k in ("rois", "rois_3d", "rois_3d_cen"):                    # one anchor grid for both images
            c[k] = np.ascontiguousarray(np.broadcast_to(c[k][None], (2,) + c[k].shape))
        scene = str(c["scene"])
        c["transforms"] = z["%s/scene_%s/transforms" % (shape, scene)].copy()
        c["transforms"][:, :, :4] = c["transforms_2d"]                  # the 2D columns are normalised with the case's own means and stds
        c["raw_gt"] = z["%s/scene_%s/raw_gt" % (shape, scene)]
        c["val_counts"] = z["%s/scene_%s/val_counts" % (shape, scene)]
        c["bbox_3d"] = c["bbox_3d"].copy()
        c["bbox_3d"][:, :, :8] *= np.float32(c["head_scale"])
        bs, ff, l2d, l3d, lah, liou, use_acc, un, dyn, has_acc = c["config"]
        c["box_samples"], c["fg_fraction"] = float(bs), float(ff)
        c["kw"] = dict(means=c["means"], stds=c["stds"], bbox_2d_lambda=float(l2d), bbox_3d_lambda=float(l3d), bbox_axis_head_lambda=float(lah),
                       iou_2d_lambda=float(liou), use_acceptance=bool(use_acc), bbox_un_lambda=float(un), bbox_un_dynamic=bool(dyn))
        if not has_acc:
            c["acceptance"] = None
    return cases


def case_ids():
    return sorted("%s/%s" % k for k in golden())


def case_of(cid):
    return golden()[tuple(cid.split("/"))]


@functools.lru_cache(maxsize=None)
def sampled(cid):
    c = case_of(cid)
    return restate_sampling(c["transforms"][:, :, 4], c["prob"], c["val_counts"], box_samples=c["box_samples"], fg_fraction=c["fg_fraction"])


@functools.lru_cache(maxsize=None)
def restated(cid):
    c, s = case_of(cid), sampled(cid)
    return restate(c["bbox_2d"], c["bbox_3d"], c["acceptance"], c["transforms"], c["raw_gt"], c["rois"], c["rois_3d"], c["rois_3d_cen"], c["p2"],
                   c["scale_factor"], s["fg_lists"], s["counts"][:, 2], state_in=tuple(c["state_in"]), **c["kw"])


@functools.lru_cache(maxsize=None)
def reference_errors(cid):
    """e_ref of a golden case: |reference - float64 restatement| of the loss, of each statistic, of each gradient (largest entry) and of
    the running weight after the step"""
    c, r = case_of(cid), restated(cid)
    e = {"loss": abs(float(c["loss"]) - r["loss"]), "weight": abs(float(c["state_out"][1]) - r["state_out"][1])}
    for k, v in zip(STAT_NAMES, c["stats"]):
        if np.isnan(v):                       # the reference did not report it: the term is absent (0 here) or no head was given
            e[k] = 0.0
        else:
            e[k] = abs(float(v) - float(r["stats"][k]))
    for k in ("grad_bbox_2d", "grad_bbox_3d", "grad_acceptance"):
        e[k] = float(np.abs(c[k].astype(np.float64) - r[k]).max())
    return e


def loss_bound(r):
    n, m = r["n"], r["mean_abs"]
    b = sum((n + GROUP_OPS[g] + 1) * m.get(g, 0.0) for g in ("2d", "3d", "bce", "un", "iou"))
    b += COMBINE_OPS * sum(m.get(g, 0.0) for g in ("2d", "3d", "bce", "un", "iou"))
    return EPS32 * b


def test_golden_holds_the_cases():
    r210 = {"both_cut", "neither", "inf", "quota_zero", "no_gt_image", "all_ignored_image", "plain", "with_2d", "static_un", "quota_zero_no_gt",
            "dyn3_s0", "dyn3_s1", "dyn3_s2"}
    r1332 = r210 - {"neither", "all_ignored_image", "static_un"}
    assert {k for k in golden()} == {("r210", n) for n in r210} | {("r1332", n) for n in r1332}
    assert case_of("r210/both_cut")["bbox_3d"].shape == (2, 210, 11) and case_of("r1332/both_cut")["bbox_2d"].shape == (2, 1332, 4)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert case_of("r210/both_cut")["scale_factor"].tolist() == [1.0, 0.8]
    # the regimes the cases are there for
    for shape in ("r210", "r1332"):
        s = sampled(shape + "/both_cut")["counts"]
        assert (s[:, 2] < s[:, 0]).all() and (s[:, 2] > 0).all()
        s = sampled(shape + "/quota_zero")["counts"]
        assert (s[:, 2] == 0).all() and (s[:, 4] == s[:, 0]).all() and (s[:, 4] > 0).all()       # active anchors, and no IoU
        assert restated(shape + "/quota_zero")["finite_iou"][1] == 0 and not restated(shape + "/quota_zero")["has_iou"]
        s = sampled(shape + "/quota_zero_no_gt")["counts"]
        assert s[0, 4] > 0 and s[1].sum() == 0
        s = sampled(shape + "/no_gt_image")["counts"]
        assert s[0, 2] > 0 and s[1, 2] == 0 and s[1, 4] == 0                                     # fg_num > 0 beside fg_num == 0
        assert not restated(shape + "/plain")["weighted"] and restated(shape + "/both_cut")["weighted"]
        assert restated(shape + "/with_2d")["stats"]["bbox_2d"] > 0
        assert [case_of("%s/dyn3_s%d" % (shape, k))["state_in"][0] for k in range(3)] == [0, 1, 2]
    assert restated("r210/static_un")["stats"]["un"] > 0 and not restated("r210/static_un")["weighted"]
    assert sampled("r210/all_ignored_image")["counts"][0].sum() == 0


@pytest.mark.parametrize("cid", case_ids())
def test_restatement_matches_the_reference(cid):
    c, r, e = case_of(cid), restated(cid), reference_errors(cid)
    # the reference's gradient on the axis column is non-zero exactly on the active anchors (axis lies strictly inside (0, 1))
    active_ref = c["grad_bbox_3d"][:, :, 8] != 0
    mine = np.zeros_like(active_ref)
    mine[r["active"]] = True
    assert np.array_equal(active_ref, mine), "the active set differs from the reference's"
    assert r["n"] > 0
    # what the generator asserted, seen from here: no isfinite filter drops anything, so the two deliberate differences cannot show
    assert r["finite_unweighted"] == [r["n"]] * 9 and r["finite_weighted"] == [r["n"]] * 7
    assert r["finite_iou"][0] == r["n"] and r["finite_iou"][1] == r["finite_iou"][2] and r["has_iou"] == (r["finite_iou"][1] > 0)
    assert float(c["state_out"][0]) == r["state_out"][0]
    n, m, st = r["n"], r["mean_abs"], r["stats"]
    bounds = {"loss": loss_bound(r), "total": loss_bound(r)}
    bounds["bbox_2d"] = EPS32 * (n + GROUP_OPS["2d"] + 1 + 4) * m.get("2d", 0.0)
    bounds["bbox_3d"] = EPS32 * ((n + GROUP_OPS["3d"] + 1 + 9) * m.get("3d", 0.0) + (n + GROUP_OPS["bce"] + 1 + 9) * m.get("bce", 0.0))
    # the weight (:1323-1341): this step's init, the nine unweighted means, enters with 1 / n_frames; the state that came in is the recorded one
    bounds["weight"] = EPS32 * (n + GROUP_OPS["bce"] + 1 + 9) * m["init"] / r["state_out"][0] if c["kw"]["bbox_un_dynamic"] else 0.0
    bounds["un"] = EPS32 * (n + GROUP_OPS["un"] + 1) * m.get("un", 0.0)
    bounds["iou_2d_los"] = EPS32 * (n + GROUP_OPS["iou"] + 1) * m.get("iou", 0.0)
    bounds["iou_2d"] = EPS32 * (n + GROUP_OPS["iou"] + 1) * st["iou_2d"]
    bounds["cen"] = EPS32 * (n + 24 + 1) * m["cen"]
    bounds["z"] = EPS32 * (n + 7 + 1) * m["z"]
    bounds["rot"] = EPS32 * (n + 8 + 1) * m["rot"]
    bounds["conf"] = EPS32 * (n + 1) * (st["conf"] if not np.isnan(st["conf"]) else 0.0)
    for k in ("axis", "head", "cen_dist_lt_0.2"):
        bounds[k] = EPS32
    for k in ("grad_bbox_2d", "grad_bbox_3d", "grad_acceptance"):
        bounds[k] = K_GRAD * EPS32 * np.abs(r[k]).max()
    for k in sorted(e):
        print("%s: e_ref %-16s %.3e  bound %.3e  (%.3f of it)" % (cid, k, e[k], bounds[k], e[k] / bounds[k] if bounds[k] else 0.0))
    for k in sorted(e):
        assert e[k] <= bounds[k], (cid, k, e[k], bounds[k])
    # gradients are 0 off the active set, in the reference as here
    for k in ("grad_bbox_2d", "grad_bbox_3d"):
        assert not c[k][~mine].any() and not r[k][~mine].any()
    assert not c["grad_bbox_3d"][:, :, 10:].any()


def test_dynamic_weight_over_three_steps():
    """:1336-1341 through one loss object: each step's state is the next one's input, and the weight follows the recorded one"""
    for shape in ("r210", "r1332"):
        prev = (0.0, 0.0)
        for k in range(3):
            cid = "%s/dyn3_s%d" % (shape, k)
            c, r = case_of(cid), restated(cid)
            assert tuple(c["state_in"]) == tuple(map(float, prev)) or k == 0
            assert r["state_out"][0] == k + 1 == c["state_out"][0]
            prev = c["state_out"]


def test_restatement_edge_rules():
    """no active anchor (:1154); an image without a quota has IoU 0 (:617); a box that misses its target: -log IoU = inf is dropped and
    its gradient is 0; a NaN element drops out of its own term only"""
    c = case_of("r210/both_cut")
    s = sampled("r210/both_cut")
    args = [c[k] for k in ("bbox_2d", "bbox_3d", "acceptance", "transforms", "raw_gt", "rois", "rois_3d", "rois_3d_cen", "p2", "scale_factor")]
    empty = [np.zeros(0, np.int64)] * 2
    r = restate(*args, empty, [0, 0], state_in=(5.0, 2.5), **c["kw"])
    assert r["loss"] == 0.0 and r["state_out"] == (5.0, 2.5) and np.isnan(r["stats"]["cen"]) and not r["grad_bbox_3d"].any()
    r0 = restated("r210/both_cut")
    r = restate(*args, s["fg_lists"], [s["counts"][0, 2], 0], state_in=(0.0, 0.0), **c["kw"])
    assert r["finite_iou"][1] == len(s["fg_lists"][0]) and not r["grad_bbox_2d"][1].any() and r["grad_bbox_2d"][0].any()
    assert r["stats"]["bbox_3d"] == r0["stats"]["bbox_3d"]
    b2 = c["bbox_2d"].copy()
    miss = s["fg_lists"][0][0]
    b2[0, miss, 0] = 40.0                                      # forty widths to the right
    a2 = list(args)
    a2[0] = b2
    r = restate(*a2, s["fg_lists"], s["counts"][:, 2], state_in=(0.0, 0.0), **c["kw"])
    assert r["finite_iou"] == (r["n"], r["n"] - 1, r["n"] - 1) and np.isfinite(r["loss"]) and not r["grad_bbox_2d"][0, miss].any()
    b3 = c["bbox_3d"].copy()
    b3[0, miss, 1] = np.nan
    a3 = list(args)
    a3[1] = b3
    r = restate(*a3, s["fg_lists"], s["counts"][:, 2], state_in=(0.0, 0.0), **c["kw"])
    assert r["finite_unweighted"] == [r["n"], r["n"] - 1] + [r["n"]] * 7 and r["finite_weighted"][1] == r["n"] - 1
    assert np.isfinite(r["loss"]) and np.isfinite(r["grad_bbox_3d"]).all() and np.isfinite(r["grad_acceptance"]).all()
    assert r["grad_bbox_3d"][0, miss, 1] == 0.0 and r["grad_bbox_3d"][0, miss, 0] != 0.0


# ---------------------------------------------------------------------------------------------- ABI and module

NEW_SYMBOLS = ("gnms_reg_loss_workspace_bytes", "gnms_reg_loss")


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
    from groomed_nms_amd import _lib, build
    assert "regression.hip" in build.SOURCES
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
    from groomed_nms_amd import regression
    assert "#define GNMS_REG_STATS %d" % regression.N_STATS in text and "#define GNMS_REG_STAT_COUNTS %d" % regression.N_STAT_COUNTS in text


def _call(lib, B=2, R=64, ld3=11, ld_tr=14, ld_gt=21, ld_rois=5, ld_r3=11, p2_rows=4, acc=True, use_acc=1, un=0.0, dyn=0, state=True,
          ws_bytes=1 << 30, null=None):
    fake = ctypes.c_void_p(1 << 20)
    v = (ctypes.c_double * 13)(*([1.0] * 13))
    host = ctypes.cast(v, ctypes.c_void_p)
    ptrs = {k: fake for k in ("bbox_2d", "bbox_3d", "transforms", "raw_gt", "rois", "rois_3d", "cen", "p2", "scale", "fg_index", "fg_counts", "counts",
                              "loss", "stats", "stat_counts", "d2", "d3", "ws")}
    ptrs["acc"] = fake if acc else None
    ptrs["dacc"] = fake if acc else None
    ptrs["state"] = fake if state else None
    if null:
        ptrs[null] = None
    return lib.gnms_reg_loss(ptrs["bbox_2d"], ptrs["bbox_3d"], ld3, ptrs["acc"], ptrs["transforms"], ld_tr, ptrs["raw_gt"], ld_gt, ptrs["rois"],
                             ld_rois, ptrs["rois_3d"], ld_r3, ptrs["cen"], ptrs["p2"], p2_rows, ptrs["scale"], ptrs["fg_index"], ptrs["fg_counts"],
                             ptrs["counts"], B, R, host, host, 0.0, 1.0, 0.35, 1.0, use_acc, un, dyn, ptrs["state"], ptrs["loss"], ptrs["stats"],
                             ptrs["stat_counts"], ptrs["d2"], ptrs["d3"], ptrs["dacc"], ptrs["ws"], ws_bytes, None)


def test_argument_errors_without_gpu(lib):
    """every check below returns before a HIP call"""
    INVALID, WORKSPACE = -1, -4            # GNMS_ERR_INVALID_ARGUMENT, GNMS_ERR_WORKSPACE
    assert _call(lib, B=0) == INVALID and _call(lib, R=0) == INVALID
    assert _call(lib, ld3=9) == INVALID and b"10 are read" in lib.gnms_last_error()
    assert _call(lib, ld_tr=13) == INVALID and b"14 are read" in lib.gnms_last_error()
    assert _call(lib, ld_gt=20) == INVALID and _call(lib, ld_rois=3) == INVALID and _call(lib, ld_r3=10) == INVALID
    assert _call(lib, p2_rows=2) == INVALID and b"p2" in lib.gnms_last_error()
    for k in ("bbox_2d", "bbox_3d", "transforms", "raw_gt", "rois", "rois_3d", "cen", "p2", "scale", "fg_index", "fg_counts", "counts", "loss",
              "stats", "stat_counts", "d2", "d3"):
        assert _call(lib, null=k) == INVALID, k
        assert b"NULL" in lib.gnms_last_error()
    assert _call(lib, acc=False, use_acc=1) == INVALID and b"acceptance" in lib.gnms_last_error()
    assert _call(lib, acc=False, use_acc=0, un=0.5) == INVALID
    assert _call(lib, acc=False, use_acc=0, dyn=1) == INVALID
    assert _call(lib, dyn=1, state=False) == INVALID and b"un_state" in lib.gnms_last_error()
    need = lib.gnms_reg_loss_workspace_bytes(2, 126720)
    assert 0 < need < 4 << 20 and lib.gnms_reg_loss_workspace_bytes(0, 5) == 0
    assert _call(lib, R=126720, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.gnms_last_error()
    assert _call(lib, R=126720, null="ws") == WORKSPACE


def test_module_surface_and_host_errors():
    import collections
    import torch
    import groomed_nms_amd
    from groomed_nms_amd import regression
    assert groomed_nms_amd.regression_loss is regression.regression_loss and "regression_loss" in regression.__all__
    assert list(regression.STAT_NAMES) == STAT_NAMES + ["bbox_un_lambda"]
    B, R = 2, 8
    S = collections.namedtuple("S", ["fg_index", "fg_counts", "counts"])
    s = S(torch.zeros((B, R), dtype=torch.int32), torch.zeros(B, dtype=torch.int32), torch.zeros((B, 6), dtype=torch.int32))
    z = lambda *shape: torch.zeros(shape)      # noqa: E731
    good = dict(bbox_2d=z(B, R, 4), bbox_3d=z(B, R, 11), acceptance=z(B, R), targets=(z(B, R, 14), z(B, R, 21)), sample=s, rois=z(B, R, 5),
                rois_3d=z(B, R, 11), rois_3d_cen=z(B, R, 2), p2=z(B, 4, 4), scale_factor=z(B), means=[0.0] * 13, stds=[1.0] * 13)
    for mode in ("orientation_bins", "infer_2d_from_3d", "has_un", "weigh_3D_regression_loss_by_gt_iou3d"):
        with pytest.raises(NotImplementedError):
            regression.regression_loss(**good, **{mode: 1})
    with pytest.raises(NotImplementedError):
        regression.regression_loss(**good, decomp_alpha=False)
    for kw in (dict(use_acceptance_prob_in_regression_loss=True), dict(bbox_un_lambda=0.5), dict(bbox_un_dynamic=True, un_state=z(2).double())):
        with pytest.raises(ValueError, match="acceptance"):
            regression.regression_loss(**dict(good, acceptance=None), **kw)
    with pytest.raises(ValueError, match="un_state"):
        regression.regression_loss(**good, bbox_un_dynamic=True)
    with pytest.raises(ValueError, match="int32"):
        regression.regression_loss(**dict(good, sample=S(s.fg_index.long(), s.fg_counts, s.counts)))
    with pytest.raises(ValueError, match="GPU"):                  # CPU tensors never reach the library
        regression.regression_loss(**good)
    for key, bad in (("bbox_2d", z(B, R, 5)), ("bbox_3d", z(B, R, 9)), ("bbox_3d", z(B, R + 1, 11)), ("acceptance", z(B, R, 1)),
                     ("targets", (z(B, R, 13), z(B, R, 21))), ("targets", (z(B, R, 14), z(B, R + 1, 21))), ("rois", z(B, R, 3)),
                     ("rois_3d", z(1, R, 11)), ("rois_3d_cen", z(B, R, 1)), ("means", [0.0] * 12),
                     ("sample", S(torch.zeros((B, R + 1), dtype=torch.int32), s.fg_counts, s.counts))):
        with pytest.raises(ValueError):
            regression.regression_loss(**dict(good, **{key: bad}))


def test_product_does_not_import_the_checker():
    src = open(os.path.join(ROOT, "groomed_nms_amd", "regression.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            mods.add((node.module or "").split(".")[0])
    assert not mods & {"oracle", "tests", "test_sampling_host", "test_regression_loss_host", "numpy"}, mods
