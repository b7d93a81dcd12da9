"""Generate tests/golden/regression.npz by RUNNING the reference's RPN_3D_loss.forward and backward (lib/loss/rpn_3d.py) on the CPU,
in the manner of make_sampling_golden.py (whose stubs, anchor grids and scenes it imports).  Runs only where the reference checkout
(abhi1kumar/groomed_nms) is; it writes data only.

Per shape (r210, r1332; B = 2): prob, the heads bbox_2d [B, R, 4], bbox_3d [B, R, 11] and acceptance [B, R], rois, rois_3d, rois_3d_cen,
p2 and the images' scale factors (image 1: 0.8).  Per scene: the rows that the reference's compute_targets returned, `transforms`
(columns 0..13) and `raw_gt`, as float32 (the loss casts them, :467-468).  The reference normalises the returned transforms in place
(:443-453), so the object kept here holds the normalised rows once forward has run.  Per case: the configuration, means and stds, the
running-weight state before and after the step, the reference's loss, statistics and the gradients of the three heads.

cls_2d_lambda = 0 throughout, so only the terms of :1154-1407 reach the heads.  The heads go in as non-leaf tensors (x * 1.0):
bbox_transform_inv scales its deltas in place (rpn_util.py:902-912).  Every stored case is asserted to have no equal keys across a
sampling cut, every active IoU finite and > 0, axis and head strictly inside (0, 1) and finite reference gradients: then neither the
NaN that the reference's backward gives to an element its isfinite filters dropped, nor the denormalised 2D prediction of its 2D term
(which only the case with 2D means 0 and stds 1 switches on) can show, and the reference alone defines the expected values.
usage: python tests/golden/make_regression_golden.py REFERENCE_CHECKOUT"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_sampling_golden as S   # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "regression.npz")
STAT_NAMES = ["bbox_2d", "bbox_3d", "un", "iou_2d_los", "cen", "cen_dist_lt_0.2", "z", "rot", "iou_2d", "axis", "head", "conf", "total"]
# config vector: box_samples, fg_fraction, bbox_2d_lambda, bbox_3d_lambda, bbox_axis_head_lambda, iou_2d_lambda,
#                use_acceptance_prob_in_regression_loss, bbox_un_lambda, bbox_un_dynamic, acceptance given
REF_CFG = dict(l2d=0.0, l3d=1.0, lah=0.35, liou=1.0, use_acc=True, un=0.0, dyn=True, acc=True)


def conf_of(anchors, means, stds, bs, ff, c):
    return S.EasyDict(lbls=S.LBLS, ilbls=S.ILBLS, anchors=anchors, bbox_means=means[None].copy(), bbox_stds=stds[None].copy(),
                      feat_stride=16, fg_fraction=ff, box_samples=bs, ign_thresh=0.5, nms_thres=0.4, fg_thresh=0.5, bg_thresh_lo=0.0,
                      bg_thresh_hi=0.5, best_thresh=0.35, hard_negatives=True, focal_loss=0, crop_size=[512, 1760], cls_2d_lambda=0,
                      iou_2d_lambda=c["liou"], bbox_2d_lambda=c["l2d"], bbox_3d_lambda=c["l3d"], bbox_axis_head_lambda=c["lah"],
                      min_gt_vis=0.65, min_gt_h=0, max_gt_h=1e9, decomp_alpha=True, use_nms_in_loss=False, has_un=False,
                      predict_acceptance_prob=c["acc"], acceptance_prob_lambda=0, boxes_for_acceptance_prob="foregrounds",
                      use_acceptance_prob_in_regression_loss=c["use_acc"], bbox_un_lambda=c["un"], bbox_un_dynamic=c["dyn"])


def main():
    if not S.REF:
        sys.exit(__doc__)
    L = S.load_reference()
    z = {}
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    scales = [1.0, 0.8]
    inf = float("inf")
    for shape, (H, W, A) in (("r210", (5, 7, 6)), ("r1332", (3, 37, 12))):
        rng = np.random.default_rng(20260 + H * W * A)
        rois, anchors = S.anchor_grid(rng, H, W, A)
        R = len(rois)
        B, C = 2, 4
        r3 = np.zeros((R, 11), np.float32)
        r3[:, :4] = rois[:, :4]
        r3[:, 4:] = anchors[rois[:, 4].astype(np.int64), 4:] + rng.normal(0, 0.05, (R, 7))
        cen = ((rois[:, :2] + rois[:, 2:4]) / 2).astype(np.float32)
        n_gt = 5 if R < 1000 else 14
        scenes = {"valid": [S.make_gts(rng, rois, n_gt, "valid"), S.make_gts(rng, rois, n_gt, "valid")]}
        scenes["no_gt"] = [scenes["valid"][0], S.make_gts(rng, rois, 0, "none")]
        scenes["all_ign"] = [S.make_gts(rng, rois, n_gt, "ignored"), scenes["valid"][1]]
        cls = torch.from_numpy(rng.normal(0, 1.5, (B, R, C)).astype(np.float32))
        prob = torch.softmax(cls, dim=2)
        bbox_2d = rng.normal(0, 0.08, (B, R, 4)).astype(np.float32)         # near the anchor: every sampled box overlaps its target
        bbox_3d = rng.normal(0, 0.2, (B, R, 11)).astype(np.float32)
        bbox_3d[:, :, 8:10] = rng.uniform(0.02, 0.98, (B, R, 2)).astype(np.float32)
        accept = rng.uniform(0.05, 1.0, (B, R)).astype(np.float32)
        means = np.round(rng.normal(0, 0.1, 13), 3)
        stds = np.round(rng.uniform(0.5, 1.5, 13), 3)
        means_2d01 = means.copy()
        stds_2d01 = stds.copy()
        means_2d01[:4] = 0.0
        stds_2d01[:4] = 1.0
        for k, v in (("prob", prob.numpy()), ("bbox_2d", bbox_2d), ("bbox_3d", bbox_3d), ("acceptance", accept), ("rois", rois), ("rois_3d", r3),
                     ("rois_3d_cen", cen), ("p2", np.stack([p2, p2])), ("scale_factor", np.array(scales))):
            z["%s/%s" % (shape, k)] = v

        plain = dict(REF_CFG, use_acc=False, dyn=False, acc=False)
        # name, scene, box_samples, fg_fraction, config, (means, stds), the scales of bbox_3d[..., :8] of the consecutive steps
        cases = [("both_cut", "valid", 0.25, 0.04, REF_CFG, (means, stds), (1.0,)),
                 ("neither", "valid", 1.0, 0.5, REF_CFG, (means, stds), (1.0,)),
                 ("inf", "valid", inf, 0.2, REF_CFG, (means, stds), (1.0,)),
                 ("quota_zero", "valid", 0.0003, 0.2, REF_CFG, (means, stds), (1.0,)),
                 ("no_gt_image", "no_gt", 0.25, 0.04, REF_CFG, (means, stds), (1.0,)),
                 ("all_ignored_image", "all_ign", 0.25, 0.04, REF_CFG, (means, stds), (1.0,)),
                 ("plain", "valid", 0.25, 0.04, plain, (means, stds), (1.0,)),
                 ("with_2d", "valid", 0.25, 0.04, dict(REF_CFG, l2d=1.0), (means_2d01, stds_2d01), (1.0,)),
                 ("static_un", "valid", 0.25, 0.04, dict(REF_CFG, use_acc=False, dyn=False, un=0.7), (means, stds), (1.0,)),
                 ("quota_zero_no_gt", "no_gt", 0.0003, 0.2, REF_CFG, (means, stds), (1.0,)),
                 ("dyn3", "valid", 0.25, 0.04, REF_CFG, (means, stds), (1.0, 1.5, 0.5))]
        if shape == "r1332":           # the size limit: the larger shape keeps one case per regime
            cases = [c for c in cases if c[0] not in ("neither", "all_ignored_image", "static_un")]
        stored_scenes = set()
        for name, scene, bs, ff, cfg, (mu, sd), steps in cases:
            imobjs = [S.EasyDict(gts=g, p2=p2.copy(), scale_factor=scales[b]) for b, g in enumerate(scenes[scene])]
            order = [b for b in range(B) if any((not g.ign) for g in scenes[scene][b])]      # the images the loop does not skip (:406)
            real_ct, real_iou = L.compute_targets, L.iou
            loss_mod = L.RPN_3D_loss(conf_of(anchors, mu, sd, bs, ff, cfg), verbose=True)
            for step, hs in enumerate(steps):
                kept, ious = [], []

                def recording(*a, **k):
                    t, o, g = real_ct(*a, **k)
                    kept.append((t, g))
                    return t, o, g

                def iou_recording(*a, **k):
                    v = real_iou(*a, **k)
                    if k.get("mode") == "list":
                        ious.append(v.detach().numpy().copy())
                    return v
                b3 = bbox_3d.copy()
                b3[:, :, :8] *= np.float32(hs)
                x2 = torch.from_numpy(bbox_2d.copy()).requires_grad_(True)
                x3 = torch.from_numpy(b3).requires_grad_(True)
                xa = torch.from_numpy(accept.copy()).requires_grad_(True)
                state_in = np.array([loss_mod.n_frames, loss_mod.bbox_un_lambda], np.float64)
                L.compute_targets, L.iou = recording, iou_recording
                try:
                    loss, stats = loss_mod(cls.clone(), prob, x2 * 1.0, x3 * 1.0, imobjs, [H, W], rois=torch.from_numpy(rois)[None].repeat(B, 1, 1),
                                           rois_3d=torch.from_numpy(r3)[None].repeat(B, 1, 1), rois_3d_cen=torch.from_numpy(cen)[None].repeat(B, 1, 1),
                                           bbox_acceptance_prob=(xa * 1.0).unsqueeze(2) if cfg["acc"] else None)
                    loss.backward()
                finally:
                    L.compute_targets, L.iou = real_ct, real_iou
                assert len(kept) == len(order)
                tr = np.zeros((B, R, 14), np.float32)
                rg = np.zeros((B, R, 21), np.float32)
                val_counts = np.zeros(B, np.int32)
                for b, (t, g) in zip(order, kept):
                    tr[b] = t[:, :14]
                    rg[b] = g[:, :21]
                    val_counts[b] = sum(1 for q in scenes[scene][b] if not q.ign)
                    assert S.cut_keys_distinct(tr[b, :, 4], prob[b].numpy(), bs, ff), "%s/%s image %d ties at a cut" % (shape, name, b)
                if scene not in stored_scenes:
                    stored_scenes.add(scene)
                    z["%s/scene_%s/transforms" % (shape, scene)] = tr
                    z["%s/scene_%s/raw_gt" % (shape, scene)] = rg
                    z["%s/scene_%s/val_counts" % (shape, scene)] = val_counts
                else:      # the same scene gives the same rows under the same means and stds in columns 4..13; the 2D columns are per case
                    assert np.array_equal(z["%s/scene_%s/raw_gt" % (shape, scene)], rg)
                    assert np.array_equal(z["%s/scene_%s/transforms" % (shape, scene)][:, :, 4:], tr[:, :, 4:])
                # (a head that no term reaches has no gradient: bbox_2d without an IoU and a 2D term, acceptance where it is not used)
                g2, g3, ga = (x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape, np.float32) for x in (x2, x3, xa))
                active = g3[:, :, 8] != 0
                assert active.any()
                for v in ious:
                    assert np.isfinite(v).all() and (v > 0).all(), "%s/%s: an active IoU is 0 or not finite: use another seed" % (shape, name)
                assert ((b3[:, :, 8:10] > 0) & (b3[:, :, 8:10] < 1)).all()
                assert np.isfinite(g2).all() and np.isfinite(g3).all() and np.isfinite(ga).all()
                st = {s["name"]: float(s["val"]) for s in stats}
                p = "%s/%s%s/" % (shape, name, "_s%d" % step if len(steps) > 1 else "")
                z[p + "scene"] = np.array(scene)
                z[p + "config"] = np.array([bs, ff, cfg["l2d"], cfg["l3d"], cfg["lah"], cfg["liou"], cfg["use_acc"], cfg["un"], cfg["dyn"], cfg["acc"]],
                                           np.float64)
                z[p + "means"] = mu
                z[p + "stds"] = sd
                z[p + "transforms_2d"] = tr[:, :, :4].copy()       # normalised with this case's 2D means and stds
                z[p + "head_scale"] = np.array(hs, np.float64)
                z[p + "state_in"] = state_in
                z[p + "state_out"] = np.array([loss_mod.n_frames, loss_mod.bbox_un_lambda], np.float64)
                z[p + "loss"] = np.array(loss.detach().numpy(), np.float32)
                z[p + "stats"] = np.array([st.get(k, np.nan) for k in STAT_NAMES], np.float64)
                z[p + "grad_bbox_2d"] = g2
                z[p + "grad_bbox_3d"] = g3
                z[p + "grad_acceptance"] = ga
                print(p, "loss %.6f" % float(loss.detach()), "active", active.sum(axis=1).tolist(), "iou calls", len(ious),
                      "state", z[p + "state_out"].tolist(), {k: round(v, 4) for k, v in st.items()})
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
