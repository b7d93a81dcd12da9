"""Times one training step of the detection loss, forward + backward, at the loss's call site: B = 2 images of
R = 36 x 32 x 110 = 126 720 anchors, C = 4 classes, 20 ground-truth objects per image, scripts/config/groumd_nms.py with all terms on
(box_samples = fg_fraction = 0.2, after-NMS rank per image, dynamic uncertainty weight).  In the same run, alternating in rounds:
  (a) loss.RPN_3D_loss eager: forward (pack_ground_truths + upload + forward_packed) and loss.backward(); (a_packed) forward_packed alone;
  (b) forward_packed + backward replayed from a graph;
  (c) the five public calls composed by hand as INTEGRATION.md described it before the module (per-image NumPy of :399-419, uploads,
      compute_targets_batched, sample_anchors, classification_loss, after_nms_loss, regression_loss, autograd's adds), eager;
      (c_device) the same from ground truths already on the device;
  (d) (c_device) replayed from a graph;
  (e) host time of pack_ground_truths + GroundTruths.to against the per-image NumPy + uploads it replaces (wall clock, synchronised).
Device time by HIP events around one step, host work included; per variant the median, minimum, 10th / 90th percentiles over all rounds
and the medians of the rounds (their range is the run-to-run spread).  The script ends itself after --limit seconds.
usage: python tools/loss_time.py [--iters K] [--rounds N] [--out FILE]  -> one JSON line."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import _lib, after_nms, heads, regression, sampling, targets  # noqa: E402
from groomed_nms_amd.loss import RPN_3D_loss, GroundTruths, pack_ground_truths  # noqa: E402

A, FH, FW, C, D3, N_OBJ = 36, 32, 110, 4, 10, 20
LBLS, ILBLS = ["Car", "Pedestrian", "Cyclist"], ["Van", "ignore"]
HEADS = ("cls", "prob", "bbox_2d", "bbox_3d", "acceptance")


class Obj(dict):
    __getattr__ = dict.__getitem__


def config(anchors):
    return Obj(lbls=LBLS, ilbls=ILBLS, anchors=anchors, bbox_means=np.zeros((1, 13)), bbox_stds=np.ones((1, 13)), feat_stride=16, fg_fraction=0.2,
               box_samples=0.2, ign_thresh=0.5, nms_thres=0.4, fg_thresh=0.5, bg_thresh_lo=0, bg_thresh_hi=0.5, best_thresh=0.35,
               hard_negatives=True, focal_loss=0, cls_2d_lambda=1, iou_2d_lambda=1, bbox_2d_lambda=0, bbox_3d_lambda=1, bbox_axis_head_lambda=0.35,
               min_gt_vis=0.65, min_gt_h=32.0, max_gt_h=384.0, decomp_alpha=True, has_un=False, predict_acceptance_prob=True,
               acceptance_prob_lambda=0, acceptance_prob_mode="likelihood", boxes_for_acceptance_prob="foregrounds",
               use_acceptance_prob_in_regression_loss=True, bbox_un_lambda=0, bbox_un_dynamic=True, use_nms_in_loss=True,
               diff_nms_temperature=0.1, after_nms_lambda=0.05, after_nms_loss_mode="rank", best_target_box_beta=0.3)


def scene(rng):
    """the configuration's 12 scales x 3 ratios of anchors, and per image 20 objects shaped like anchors (two of an ignored class, one
    barely visible)"""
    hs = 32.0 * (384.0 / 32.0) ** (np.arange(12) / 11.0)
    anchors = np.zeros((A, 11))
    for i, (h, ratio) in enumerate((h, r) for h in hs for r in (0.5, 1.0, 1.5)):
        w = h * ratio
        anchors[i, :4] = (-w / 2 + 8, -h / 2 + 8, w / 2 + 8, h / 2 + 8)
        anchors[i, 4:] = (20.0 * 64 / h, 1.6, 1.5, 3.9, 0.0, 0.0, 1.0)
    imobjs = []
    for b in range(2):
        gts = []
        for j in range(N_OBJ):
            h = float(rng.uniform(40, 300))
            w = h * float(rng.uniform(0.5, 1.5))
            x, y = float(rng.uniform(0, 1760 - w)), float(rng.uniform(0, 512 - min(h, 500)))
            b3 = np.concatenate([[x + w / 2, y + h / 2, rng.uniform(5, 50), 1.6, 1.5, 3.9], rng.uniform(-3, 3, 8), rng.integers(0, 2, 2)]).astype(np.float64)
            gts.append(Obj(cls="Van" if j % 10 == 3 else LBLS[j % 3], ign=False, visibility=0.3 if j == 7 else 1.0, trunc=0.0,
                           bbox_full=np.array([x, y, w, h]), bbox_3d=b3))
        imobjs.append(Obj(gts=gts, p2=np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]]), scale_factor=1.0))
    return anchors, imobjs


def numpy_ground_truths(imobjs, conf, dev):
    """lib/loss/rpn_3d.py:399-419 per image in NumPy, padded, and the uploads: what INTEGRATION.md asked of the caller"""
    B = len(imobjs)
    rows = []
    for imobj in imobjs:
        gts = imobj.gts
        igns = np.array([bool(g.ign) or g.visibility < conf.min_gt_vis or g.bbox_full[3] < conf.min_gt_h or g.cls in conf.ilbls for g in gts])
        rmvs = np.array([g.cls not in (conf.lbls + conf.ilbls) for g in gts])
        box = np.array([g.bbox_full for g in gts], np.float64).reshape(-1, 4).copy()
        box[:, 2] += box[:, 0] - 1
        box[:, 3] += box[:, 1] - 1
        val, ign = ~rmvs & ~igns, ~rmvs & igns
        b3 = np.array([g.bbox_3d for g in gts]).reshape(-1, 16)
        rows.append((box[val], box[ign], b3[val], np.array([conf.lbls.index(g.cls) + 1 for g, v in zip(gts, val) if v], np.int32)))
    M, K = max(1, max(len(r[0]) for r in rows)), max(1, max(len(r[1]) for r in rows))
    gv, gi, g3, lb = np.zeros((B, M, 4)), np.zeros((B, K, 4)), np.zeros((B, M, 16)), np.zeros((B, M), np.int32)
    for b, r in enumerate(rows):
        gv[b, :len(r[0])], gi[b, :len(r[1])], g3[b, :len(r[2])], lb[b, :len(r[3])] = r
    vc, ic = np.array([len(r[0]) for r in rows], np.int32), np.array([len(r[1]) for r in rows], np.int32)
    p2, sc = np.stack([im.p2 for im in imobjs]), np.array([im.scale_factor for im in imobjs], np.float64)
    return {k: torch.from_numpy(v).to(dev) for k, v in dict(gts_val=gv, gts_ign=gi, gts_3d=g3, box_lbls=lb, val_counts=vc, ign_counts=ic, p2=p2, scale_factor=sc).items()}


def measure(variants, iters, rounds, warm=3):
    """-> {name: median / min / p10 / p90 over all rounds and the rounds' medians}; the variants alternate round by round"""
    ts = {name: [] for name in variants}
    for name, fn in variants.items():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            one = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                one.append(e0.elapsed_time(e1) * 1e3)
            ts[name].append(one)
    out = {}
    for name, per_round in ts.items():
        v = sorted(t for one in per_round for t in one)
        out[name + "_us"] = dict(median=round(statistics.median(v), 1), min=round(v[0], 1), p10=round(v[len(v) // 10], 1), p90=round(v[(len(v) * 9) // 10], 1),
                                 round_medians=[round(statistics.median(one), 1) for one in per_round])
    return out


def graph_of(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40, help="steps per variant and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="seconds after which the script ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(11)
    anchors, imobjs = scene(rng)
    conf = config(anchors)
    B, R = 2, A * FH * FW
    rois, rois_3d, cen = heads.anchor_grid(anchors, (FH, FW), 16, batch=B, device=dev)
    f = np.float32
    cls = rng.normal(0, 1.5, (B, R, C)).astype(f)
    d = dict(cls=cls, prob=torch.softmax(torch.from_numpy(cls), 2).numpy(), bbox_2d=rng.normal(0, 0.08, (B, R, 4)).astype(f),
             bbox_3d=rng.normal(0, 0.2, (B, R, D3)).astype(f), acceptance=rng.uniform(0.05, 1.0, (B, R, 1)).astype(f))
    d["bbox_3d"][:, :, 8:10] = rng.uniform(0.02, 0.98, (B, R, 2)).astype(f)
    data = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    means, stds = conf.bbox_means[0], conf.bbox_stds[0]

    def leaves():
        # leaves of the step's own: one kept across steps carries a gradient accumulator bound to the stream of its first use
        return {k: data[k].detach().requires_grad_(True) for k in HEADS}

    module = RPN_3D_loss(conf)
    gt_dev = GroundTruths.empty(B, module.capacity, device=dev)

    def a_module():
        x = leaves()
        loss, stats = module(x["cls"], x["prob"], x["bbox_2d"], x["bbox_3d"], imobjs, [FH, FW], rois, rois_3d, cen, x["acceptance"])
        loss.backward()
        return loss, x

    def a_packed():
        x = leaves()
        loss, stats = module.forward_packed(x["cls"], x["prob"], x["bbox_2d"], x["bbox_3d"], gt_dev, rois, rois_3d, cen, x["acceptance"])
        loss.backward()
        return loss, x

    state = regression.new_un_state(dev)

    def hand(g, x):
        t = targets.compute_targets_batched(rois, g["gts_val"], g["box_lbls"], conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                                            conf.best_thresh, gts_ign=g["gts_ign"], val_counts=g["val_counts"], ign_counts=g["ign_counts"],
                                            gts_3d=g["gts_3d"], rois_3d=rois_3d, rois_3d_cen=cen, anchor_cols=anchors.shape[1], means=conf.bbox_means,
                                            stds=conf.bbox_stds, want=("transforms", "raw_gt"))
        s = sampling.sample_anchors(t.transforms[..., 4], x["prob"], g["val_counts"], box_samples=conf.box_samples, fg_fraction=conf.fg_fraction)
        loss, _ = sampling.classification_loss(x["cls"], s, fg_fraction=conf.fg_fraction, focal_loss=0, cls_2d_lambda=1)
        acc = x["acceptance"][:, :, 0]
        l_nms, _ = after_nms.after_nms_loss(x["prob"], acc, x["bbox_2d"], x["bbox_3d"], t, s, rois, rois_3d, cen, g["p2"], g["scale_factor"], g["gts_val"],
                                            g["gts_3d"], g["val_counts"], means=means, stds=stds, after_nms_lambda=0.05, temperature=0.1)
        loss = loss + l_nms
        l_reg, _ = regression.regression_loss(x["bbox_2d"], x["bbox_3d"], acc, t, s, rois, rois_3d, cen, g["p2"], g["scale_factor"], means=means, stds=stds,
                                              bbox_2d_lambda=0, bbox_3d_lambda=1, bbox_axis_head_lambda=0.35, iou_2d_lambda=1,
                                              use_acceptance_prob_in_regression_loss=True, bbox_un_dynamic=True, un_state=state)
        loss = loss + l_reg
        loss.backward()
        return loss, x

    def c_hand():
        return hand(numpy_ground_truths(imobjs, conf, dev), leaves())

    g_static = numpy_ground_truths(imobjs, conf, dev)

    def c_device():
        return hand(g_static, leaves())

    # the two routes compute the same step
    pack_ground_truths(imobjs, LBLS, ILBLS, capacity=module.capacity).to(dev, out=gt_dev)
    la, xa = a_module()
    lc, xc = c_hand()
    torch.cuda.synchronize()
    line = dict(B=B, R=R, C=C, objects_per_image=N_OBJ, iters=args.iters, rounds=args.rounds, total_module=float(la.detach().cpu()),
                total_hand=float(lc.detach().cpu()), gradients_equal=all(torch.equal(xa[k].grad, xc[k].grad) for k in HEADS if xc[k].grad is not None),
                sampled_foreground=module.last_sample.fg_counts.tolist(), val_counts=module.last_ground_truths["val_counts"].tolist())
    gb, gd = graph_of(a_packed), graph_of(c_device)
    line.update(measure({"a_module_eager": a_module, "a_packed_eager": a_packed, "b_module_graph": gb.replay, "c_hand_eager": c_hand,
                         "c_device_hand_eager": c_device, "d_hand_graph": gd.replay}, args.iters, args.rounds))

    def host_us(fn, n=200):
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        ts.sort()
        return dict(median=round(statistics.median(ts), 1), min=round(ts[0], 1), p90=round(ts[(n * 9) // 10], 1))
    line["e_pack_and_upload_host_us"] = host_us(lambda: pack_ground_truths(imobjs, LBLS, ILBLS, capacity=module.capacity).to(dev, out=gt_dev))
    line["e_numpy_and_uploads_host_us"] = host_us(lambda: numpy_ground_truths(imobjs, conf, dev))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
