"""Times the after-NMS block of the RPN loss (groomed_nms_amd/after_nms.py) at the loss's call site: B = 2 images of
R = 32 * 110 * 36 = 126 720 anchors, the reference's configuration (rank per image, lambda 0.05, linear pruning, masked groups of 100),
12 ground truths per image, a sampled foreground of a few thousand anchors per image clustered on the ground truths (the quota of
box_samples = 0.2), of which the 500 best go through the NMS.  In the same run:
  (a) after_nms_loss forward + backward (the gradient of the acceptance head comes out of the call), eager and replayed from a graph;
  (b) what a user assembles from the entries this package had before: a stock-torch decode of ALL anchors (2D boxes and cuboids),
      proposals.select_topk, torch gathers, proposals.training_tail and autograd's scatter back into acceptance.  (b) ranks only the
      boxes that went through the NMS: it has no zero tail, so its loss is a different (wrong) number for more than 500 foreground anchors.
Device time by HIP events around one step, host work included; median, minimum and the 10th / 90th percentiles of --iters steps after a
warm-up.  The script ends itself after --limit seconds.
usage: python tools/after_nms_time.py [--iters K] [--out FILE]  -> one JSON line."""
import argparse
import collections
import json
import math
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import after_nms, proposals, _lib  # noqa: E402

R, D3, M, K = 126720, 11, 12, 500
Sample = collections.namedtuple("Sample", ["fg_index", "fg_counts", "counts"])


def spread_us(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return dict(median=round(statistics.median(ts), 1), min=round(ts[0], 1), p10=round(ts[len(ts) // 10], 1), p90=round(ts[(len(ts) * 9) // 10], 1))


def scene(rng, B, n_fg, dev):
    """anchors whose decoded boxes lie on the ground truths for the sampled foreground, anywhere for the rest"""
    f = np.float32
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    xy, wh = rng.uniform(0, 1700, (B, R, 2)), rng.uniform(16, 90, (B, R, 2))
    gts_val, gts_3d = np.zeros((B, M, 4)), np.zeros((B, M, 16))
    raw_gt = np.zeros((B, R, 21), f)
    raw_gt[:, :, 19:21] = rng.integers(0, 2, (B, R, 2))
    z_anchor = rng.uniform(5, 40, (B, R, 1))
    idx = np.full((B, R), -1, np.int32)
    counts = np.zeros((B, 6), np.int32)
    for b in range(B):
        gxy, gwh = rng.uniform(100, 1500, (M, 2)), rng.uniform(40, 120, (M, 2))
        gts_val[b] = np.concatenate([gxy, gxy + gwh], 1)
        fg = np.sort(rng.choice(R, n_fg, replace=False))
        own = rng.integers(0, M, n_fg)
        wh[b, fg] = gwh[own] * rng.uniform(0.8, 1.25, (n_fg, 2))
        xy[b, fg] = gxy[own] + rng.normal(0, 6, (n_fg, 2))
        gz = rng.uniform(8, 40, M)
        z_anchor[b, fg, 0] = gz[own] + rng.normal(0, 0.3, n_fg)
        c = gxy + gwh / 2
        z3 = gz - p2[2, 3]
        gts_3d[b, :, 7] = ((z3 + p2[2, 3]) * c[:, 0] - p2[0, 2] * z3 - p2[0, 3]) / p2[0, 0]
        gts_3d[b, :, 8] = ((z3 + p2[2, 3]) * c[:, 1] - p2[1, 2] * z3 - p2[1, 3]) / p2[1, 1]
        gts_3d[b, :, 9] = z3
        gts_3d[b, :, 3:6] = [1.6, 1.5, 3.9]
        gts_3d[b, :, 10] = rng.uniform(-3, 3, M)
        idx[b, :n_fg] = fg
        counts[b, 2] = counts[b, 4] = n_fg
    d = dict(rois=np.concatenate([xy, xy + wh, rng.integers(0, 36, (B, R, 1))], 2).astype(f))
    d["rois_3d"] = np.concatenate([d["rois"][:, :, :4], z_anchor, np.tile([1.6, 1.5, 3.9], (B, R, 1)), rng.uniform(-3, 3, (B, R, 3))], 2).astype(f)
    d["rois_3d_cen"] = (xy + wh / 2).astype(f)
    d["bbox_2d"] = rng.normal(0, 0.05, (B, R, 4)).astype(f)
    d["bbox_3d"] = rng.normal(0, 0.05, (B, R, D3)).astype(f)
    d["acceptance"] = rng.uniform(0.05, 1.0, (B, R)).astype(f)
    prob = rng.uniform(0.01, 1, (B, R, 4))
    d["prob"] = (prob / prob.sum(2, keepdims=True)).astype(f)
    d["raw_gt"] = raw_gt
    d["p2"] = np.stack([p2] * B)
    d["scale_factor"] = np.ones(B)
    d["gts_val"], d["gts_3d"] = gts_val, gts_3d
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    t["val_counts"] = torch.full((B,), M, dtype=torch.int32, device=dev)
    s = Sample(torch.from_numpy(idx).to(dev), torch.from_numpy(counts[:, 4].copy()).to(dev), torch.from_numpy(counts).to(dev))
    return t, s


def torch_decode_all(t, means, stds):
    """the loss's decode of every anchor in stock torch (:316-363, :532-574): what stands in front of select_topk without gnms_after_nms_decode"""
    rois, b2, b3, r3, gt = t["rois"], t["bbox_2d"], t["bbox_3d"], t["rois_3d"], t["raw_gt"]
    w = rois[..., 2] - rois[..., 0] + 1.0
    h = rois[..., 3] - rois[..., 1] + 1.0
    cx, cy = rois[..., 0] + 0.5 * w, rois[..., 1] + 0.5 * h
    dx, dy, dw, dh = (b2[..., k] * stds[k] + means[k] for k in range(4))
    px, py, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    boxes = torch.stack([px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw - 1, py + 0.5 * ph - 1], -1)
    dn = lambda k, col: b3[..., col] * stds[k] + means[k]           # noqa: E731
    x_dn, y_dn = dn(4, 0) * w + t["rois_3d_cen"][..., 0], dn(5, 1) * h + t["rois_3d_cen"][..., 1]
    z_dn = r3[..., 4] + dn(6, 2)
    whl = [torch.exp(dn(7 + k, 3 + k)) * r3[..., 5 + k] for k in range(3)]
    rsin, rcos = r3[..., 9] + dn(11, 6), r3[..., 10] + dn(12, 7)
    P, sc = t["p2"].float(), t["scale_factor"].float()[:, None]
    z = z_dn - P[:, 2, 3, None]
    x = ((z + P[:, 2, 3, None]) * (x_dn / sc) - P[:, 0, 2, None] * z - P[:, 0, 3, None]) / P[:, 0, 0, None]
    y = ((z + P[:, 2, 3, None]) * (y_dn / sc) - P[:, 1, 2, None] * z - P[:, 1, 3, None]) / P[:, 1, 1, None]
    rot = torch.where(gt[..., 19] == 1, rsin, rcos)
    rot = torch.where(gt[..., 20] == 1, rot + math.pi, rot)
    ry = rot + torch.atan2(-z, x) + 0.5 * math.pi
    for _ in range(2):
        ry = torch.where(ry > math.pi, ry - 2 * math.pi, ry)
        ry = torch.where(ry <= -math.pi, ry + 2 * math.pi, ry)
    return boxes, torch.stack([x, y, z] + whl + [ry], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--fg", type=int, default=3000, help="sampled foreground anchors per image")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the script ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    _lib.load()
    dev = torch.device("cuda")
    B = 2
    rng = np.random.default_rng(7)
    t, s = scene(rng, B, args.fg, dev)
    means, stds = [0.0] * 13, [1.0] * 13
    kw = dict(means=means, stds=stds, after_nms_lambda=0.05, temperature=0.1, max_nms_boxes=K)
    acc_data = t["acceptance"].clone()

    def ours():
        # a leaf of this step's own: a leaf kept across steps carries a gradient accumulator bound to the stream of its first use, and a
        # captured backward must not meet one that lives on the default stream
        acc = acc_data.detach().requires_grad_(True)
        loss, info = after_nms.after_nms_loss(t["prob"], acc, t["bbox_2d"], t["bbox_3d"], (None, t["raw_gt"]), s, t["rois"], t["rois_3d"],
                                              t["rois_3d_cen"], t["p2"], t["scale_factor"], t["gts_val"], t["gts_3d"], t["val_counts"], **kw)
        (g,) = torch.autograd.grad(loss, acc)
        return loss, g, info
    loss, g, info = ours()
    line = dict(B=B, R=R, fg_per_image=args.fg, selected=info["sel_counts"].tolist(), targets=int(info["targets_after_nms"].sum()),
                loss=float(loss.detach().cpu()), iters=args.iters)
    line["a_after_nms_loss_eager_us"] = spread_us(ours, args.iters)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ours()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ours()
    line["a_after_nms_loss_graph_us"] = spread_us(graph.replay, args.iters)

    gt_params = t["gts_3d"][:, :, [7, 8, 9, 3, 4, 5, 10]].float().contiguous()
    gt_boxes = t["gts_val"].float().contiguous()

    def parent():
        acc = acc_data.detach().requires_grad_(True)
        boxes, cub = torch_decode_all(t, means, stds)
        idx, num, _, _ = proposals.select_topk(acc.detach(), K, candidates=s.fg_index, candidate_counts=s.fg_counts)
        ix = idx.clamp(min=0)
        sel_scores = torch.gather(acc, 1, ix)
        sel_boxes = torch.gather(boxes, 1, ix[:, :, None].expand(B, K, 4))
        sel_cub = torch.gather(cub, 1, ix[:, :, None].expand(B, K, 7)).contiguous()
        lb, _, _ = proposals.training_tail(sel_scores, sel_boxes, sel_cub, gt_params, gt_boxes, 0.3, counts=num, gt_counts=t["val_counts"],
                                           temperature=0.1)
        l = 0.05 * lb.sum() / B
        (g,) = torch.autograd.grad(l, acc)
        return l, g
    try:
        lp, _ = parent()
        line["b_parent_entries_loss_without_tail"] = float(lp.detach().cpu())
        line["b_parent_entries_us"] = spread_us(parent, args.iters)
    except _lib.GnmsError as e:                         # (training_tail needs the C++ binding)
        line["b_parent_entries_us"] = "not run: %s" % e
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
