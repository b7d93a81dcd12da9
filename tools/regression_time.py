"""Times the box regression, 2D IoU and uncertainty terms of the RPN loss (gnms_reg_loss, csrc/regression.hip) at the loss's call site:
R = 32 * 110 * 36 = 126 720 anchors per image, about 1 % of them sampled foreground, B = 2 and 8, the reference's configuration
(iou_2d_lambda = bbox_3d_lambda = 1, bbox_axis_head_lambda = 0.35, acceptance weighting, dynamic uncertainty weight).
Reports per shape: the device time of one regression_loss call (HIP events around one call: the launches and the wrapper's host work;
median and minimum of --iters calls after a warm-up), the same replayed from a captured graph (no host work between the launches), and,
on the same box in the same run, a stock-torch transcription of lib/loss/rpn_3d.py:316-363, :532-577, :617-621 and :1154-1407 on GPU
tensors -- forward with the reference's three host reads, and backward -- which is what a user of this package runs today.  The
algorithmic bytes: the three dense gradients written once (B R (4 + D3 + 1) floats) plus the active anchors' rows gathered twice.
The script ends itself after --limit seconds.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` with --iters 20
--no-torch, a run of its own (profiles/README.md).
usage: python tools/regression_time.py [--iters K] [--out FILE] [--no-torch]  -> one JSON line per shape."""
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import regression, _lib  # noqa: E402

R, D3 = 126720, 11
PEAK = 8.0e12
ROW_FLOATS = 4 + D3 + 1 + 14 + 21 + 5 + 11 + 2            # what one active anchor gathers
Sample = collections.namedtuple("Sample", ["fg_index", "fg_counts", "counts"])


def median_us(fn, iters, warm=5):
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
    return statistics.median(ts), min(ts)


def scene(rng, B, dev):
    f = np.float32
    xy, wh = rng.uniform(0, 1700, (B, R, 2)), rng.uniform(16, 90, (B, R, 2))
    d = dict(rois=np.concatenate([xy, xy + wh, rng.integers(0, 36, (B, R, 1))], 2).astype(f))
    d["rois_3d"] = np.concatenate([d["rois"][:, :, :4], rng.uniform(5, 40, (B, R, 1)), rng.uniform(0.5, 4, (B, R, 3)), rng.uniform(-3, 3, (B, R, 3))], 2).astype(f)
    d["rois_3d_cen"] = (xy + wh / 2).astype(f)
    d["bbox_2d"] = rng.normal(0, 0.1, (B, R, 4)).astype(f)
    d["bbox_3d"] = rng.normal(0, 0.5, (B, R, D3)).astype(f)
    d["bbox_3d"][:, :, 8:10] = rng.uniform(0.02, 0.98, (B, R, 2))
    d["acceptance"] = rng.uniform(0.05, 1.0, (B, R)).astype(f)
    d["transforms"] = rng.normal(0, 0.3, (B, R, 14)).astype(f)
    d["transforms"][:, :, :4] = rng.normal(0, 0.1, (B, R, 4))
    d["raw_gt"] = rng.uniform(-3, 3, (B, R, 21)).astype(f)
    d["raw_gt"][:, :, 19:21] = rng.integers(0, 2, (B, R, 2))
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    d["p2"] = np.stack([p2] * B)
    d["scale_factor"] = np.ones(B)
    active = rng.random((B, R)) < 0.01
    idx = np.full((B, R), -1, np.int32)
    counts = np.zeros((B, 6), np.int32)
    for b in range(B):
        l = np.flatnonzero(active[b])
        idx[b, :len(l)] = l
        counts[b, 2] = counts[b, 4] = len(l)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    s = Sample(torch.from_numpy(idx).to(dev), torch.from_numpy(counts[:, 4].copy()).to(dev), torch.from_numpy(counts).to(dev))
    return t, s, torch.from_numpy(active).to(dev), int(active.sum())


def decode_2d(rois, deltas, means, stds):
    """bbox_transform_inv (rpn_util.py:886-934) without its in-place scaling"""
    w = rois[..., 2] - rois[..., 0] + 1.0
    h = rois[..., 3] - rois[..., 1] + 1.0
    cx, cy = rois[..., 0] + 0.5 * w, rois[..., 1] + 0.5 * h
    dx, dy, dw, dh = (deltas[..., k] * stds[k] + means[k] for k in range(4))
    px, py, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw - 1, py + 0.5 * ph - 1], -1)


def stock_torch(t, active, means, stds, state, l3d=1.0, lah=0.35, liou=1.0):
    """the reference's sequence of masked operations on GPU tensors, host reads included (np.sum(bbox_weights), the axis accuracy's
    .cpu().numpy(), the running weight's .item()); returns (loss, stats)"""
    b2, b3, acc = t["bbox_2d"], t["bbox_3d"], t["acceptance"].reshape(-1)
    tr, gt, rois, r3 = t["transforms"], t["raw_gt"], t["rois"], t["rois_3d"]
    stats = {}
    coords = decode_2d(rois, b2, means, stds)                                              # :316
    coords_tar = decode_2d(rois, tr[..., :4], means, stds)                                 # :523
    w = rois[..., 2] - rois[..., 0] + 1.0
    h = rois[..., 3] - rois[..., 1] + 1.0
    x_dn = (b3[..., 0] * stds[4] + means[4]) * w + t["rois_3d_cen"][..., 0]                # :318-357
    y_dn = (b3[..., 1] * stds[5] + means[5]) * h + t["rois_3d_cen"][..., 1]
    z_dn = r3[..., 4] + (b3[..., 2] * stds[6] + means[6])
    rsin_dn = r3[..., 9] + (b3[..., 6] * stds[11] + means[11])
    rcos_dn = r3[..., 10] + (b3[..., 7] * stds[12] + means[12])
    P = t["p2"].float()
    z_raw = z_dn - P[:, 2, 3, None]                                                        # :553-555
    x_raw = ((z_raw + P[:, 2, 3, None]) * (x_dn / t["scale_factor"].float()[:, None]) - P[:, 0, 2, None] * z_raw - P[:, 0, 3, None]) / P[:, 0, 0, None]
    y_raw = ((z_raw + P[:, 2, 3, None]) * (y_dn / t["scale_factor"].float()[:, None]) - P[:, 1, 2, None] * z_raw - P[:, 1, 3, None]) / P[:, 1, 1, None]
    sin_mask, head_mask = gt[..., 19] == 1, gt[..., 20] == 1                               # :562-571
    rot = torch.where(sin_mask, rsin_dn, rcos_dn)
    rot = torch.where(head_mask, rot + math.pi, rot).detach()
    for _ in range(2):                                                                     # snap_to_pi: the angles here need one trip
        rot = torch.where(rot > math.pi, rot - 2 * math.pi, rot)
        rot = torch.where(rot <= -math.pi, rot + 2 * math.pi, rot)
    abs_err_z = (z_raw.detach() - gt[..., 14]).abs()
    abs_err_rot = (rot - gt[..., 11]).abs()
    ious = torch.zeros_like(active, dtype=torch.float32)                                   # :617-621, per image
    for b in range(active.shape[0]):
        m = active[b]
        a_, b_ = coords[b][m], coords_tar[b][m]
        inter = torch.clamp(torch.min(a_[:, 2:], b_[:, 2:]) - torch.max(a_[:, :2], b_[:, :2]), 0)
        inter = inter[:, 0] * inter[:, 1]
        union = (a_[:, 2] - a_[:, 0]) * (a_[:, 3] - a_[:, 1]) + (b_[:, 2] - b_[:, 0]) * (b_[:, 3] - b_[:, 1]) - inter
        ious[b, m] = inter / union
    bbox_weights = active.float()
    loss = torch.zeros((), device=b2.device)
    if float(bbox_weights.sum().cpu()) > 0:                                                # :1154 (np.sum on the host)
        bw = bbox_weights.view(-1)
        act = bw > 0
        cen = torch.sqrt((x_raw.reshape(-1)[act] - gt[..., 12].reshape(-1)[act]) ** 2 + (y_raw.reshape(-1)[act] - gt[..., 13].reshape(-1)[act]) ** 2
                         + (z_raw.reshape(-1)[act] - gt[..., 14].reshape(-1)[act]) ** 2)   # :1202-1209
        stats["cen"] = cen.mean().detach()
        stats["cen_dist_lt_0.2"] = (cen <= 0.2).float().mean().detach()
        terms = [F.smooth_l1_loss(b3[..., k].reshape(-1)[act], tr[..., 5 + k].reshape(-1)[act], reduction="none") for k in range(6)]    # :1232-1237
        l_sin = F.smooth_l1_loss(b3[..., 6].reshape(-1)[act], tr[..., 12].reshape(-1)[act], reduction="none")                            # :1281-1287
        l_cos = F.smooth_l1_loss(b3[..., 7].reshape(-1)[act], tr[..., 13].reshape(-1)[act], reduction="none")
        terms.append(torch.where(sin_mask.reshape(-1)[act], l_sin, l_cos))
        l_axis = F.binary_cross_entropy(b3[..., 8].reshape(-1)[act], gt[..., 19].reshape(-1)[act], reduction="none")
        l_head = F.binary_cross_entropy(b3[..., 9].reshape(-1)[act], gt[..., 20].reshape(-1)[act], reduction="none")
        pts, lbl = b3[..., 8].reshape(-1)[act].detach().cpu().numpy(), gt[..., 19].reshape(-1)[act].cpu().numpy()                         # :1290-1297
        stats["axis"] = ((pts >= 0.5) == lbl).mean()
        pts, lbl = b3[..., 9].reshape(-1)[act].detach().cpu().numpy(), gt[..., 20].reshape(-1)[act].cpu().numpy()
        stats["head"] = ((pts >= 0.5) == lbl).mean()
        terms = [x * bw[act] for x in terms]                                               # :1299-1309
        l_axis, l_head = l_axis * bw[act], l_head * bw[act]
        init = float(sum(x[torch.isfinite(x)].mean() for x in terms).detach().item()) * l3d         # :1323-1341
        init += float((l_axis[torch.isfinite(l_axis)].mean() + l_head[torch.isfinite(l_head)].mean()).detach().item()) * lah
        if state[0] == 0:
            state[1], state[0] = init, 1
        else:
            state[0] = min(100, state[0] + 1)
            state[1] = init / state[0] + state[1] * (state[0] - 1) / state[0]
        terms = [x * acc[act] for x in terms]                                              # :1344-1356
        l_axis, l_head = l_axis * acc[act], l_head * acc[act]
        stats["conf"] = acc[act].mean().detach()
        l3 = sum(x[torch.isfinite(x)].mean() for x in terms) + (l_axis.mean() + l_head.mean()) * lah                                     # :1358-1369
        l3 = l3 * l3d
        loss = loss + l3
        stats["bbox_3d"] = l3.detach()
        if state[1] > 0:                                                                   # :1375-1382
            l_un = (1 - acc[act]).mean() * state[1]
            loss = loss + l_un
            stats["un"] = l_un.detach()
        stats["z"] = abs_err_z.reshape(-1)[act].mean()                                     # :1384-1392
        stats["rot"] = abs_err_rot.reshape(-1)[act].mean()
        iv = ious.view(-1)
        stats["iou_2d"] = iv[act & torch.isfinite(iv)].detach().mean()
        if liou and (iv[act] != 0).any():                                                  # :1395-1405 (a host read of its own)
            l_iou = -torch.log(iv[act]) * bw[act]
            l_iou = l_iou[torch.isfinite(l_iou)].mean() * liou
            loss = loss + l_iou
            stats["iou_2d_los"] = l_iou.detach()
        stats["total"] = loss.detach()
    return loss, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the script ends itself")
    ap.add_argument("--no-torch", action="store_true", help="skip the stock-torch transcription (kernel-trace runs)")
    args = ap.parse_args()
    signal.alarm(args.limit)
    _lib.load()
    dev = torch.device("cuda")
    lines = []
    for B in (2, 8):
        rng = np.random.default_rng(B)
        t, s, active, n = scene(rng, B, dev)
        means, stds = [round(float(v), 3) for v in rng.normal(0, 0.1, 13)], [round(float(v), 3) for v in rng.uniform(0.5, 1.5, 13)]
        kw = dict(means=means, stds=stds, bbox_2d_lambda=0.0, bbox_3d_lambda=1.0, bbox_axis_head_lambda=0.35, iou_2d_lambda=1.0,
                  use_acceptance_prob_in_regression_loss=True, bbox_un_dynamic=True)
        heads = [t[k].clone().requires_grad_(True) for k in ("bbox_2d", "bbox_3d", "acceptance")]
        state = regression.new_un_state(dev)

        def ours():
            return regression.regression_loss(*heads, (t["transforms"], t["raw_gt"]), s, t["rois"], t["rois_3d"], t["rois_3d_cen"], t["p2"],
                                              t["scale_factor"], un_state=state, **kw)

        def ours_fb():
            for x in heads:
                x.grad = None
            ours()[0].backward()
        loss, stats = ours()
        us_f, min_f = median_us(ours, args.iters)
        us_fb, min_fb = median_us(ours_fb, args.iters)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ours()
        us_g, min_g = median_us(graph.replay, args.iters)
        nbytes = B * R * (4 + D3 + 1) * 4 + 2 * n * ROW_FLOATS * 4
        line = dict(B=B, R=R, active=n, regression_loss_us=round(us_f, 2), regression_loss_min_us=round(min_f, 2),
                    with_backward_us=round(us_fb, 2), with_backward_min_us=round(min_fb, 2), graph_us=round(us_g, 2), graph_min_us=round(min_g, 2),
                    MB=round(nbytes / 1e6, 2), graph_fraction_of_8TBs=round(nbytes / (us_g * 1e-6) / PEAK, 4), loss=float(loss.detach().cpu()),
                    iters=args.iters)
        if not args.no_torch:
            tstate = [0, 0.0]
            th = {k: t[k].clone().requires_grad_(True) for k in ("bbox_2d", "bbox_3d", "acceptance")}

            def stock():
                for x in th.values():
                    x.grad = None
                l, _ = stock_torch(dict(t, **th), active, means, stds, tstate)
                l.backward()
                return l

            def stock_fwd():
                with torch.no_grad():
                    return stock_torch(dict(t, **th), active, means, stds, tstate)[0]
            l0 = stock()
            us_t, min_t = median_us(stock, args.iters)
            us_tf, min_tf = median_us(stock_fwd, args.iters)
            line.update(stock_torch_forward_backward_us=round(us_t, 2), stock_torch_forward_backward_min_us=round(min_t, 2),
                        stock_torch_forward_us=round(us_tf, 2), stock_torch_forward_min_us=round(min_tf, 2), stock_torch_loss=float(l0.detach().cpu()),
                        stock_torch_over_ours=round(us_t / us_fb, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
