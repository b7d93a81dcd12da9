"""Times detect.detections_from_heads at the reference's operating point (A = 126 720 anchors, 3000 -> 500 boxes, GrooMeD-NMS on the 2D
overlaps) for B = 1 and B = 2, and beside it a baseline on the same device: the reference's op sequence for the same inputs
(lib/rpn_util.py:1087-1356) written as stock torch ops on the GPU plus its NumPy half, host copies included, feeding the same NMS
layer.  Host wall time per call (synchronised), median after warm-up; one JSON line per configuration.

    python tools/detect3d_time.py [--reps 50] [--out profiles/detect3d_time.jsonl]
    rocprofv3 --kernel-trace --stats -- python tools/detect3d_time.py --reps 20 --only ours     (device time per kernel, a run of its own)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import groomed_nms_amd as G  # noqa: E402
from groomed_nms_amd import detect, synthetic  # noqa: E402
from groomed_nms_amd.groomed_nms import counts_to_host  # noqa: E402


def baseline(t, d, sf, hw):
    """the reference's sequence, image by image: ~40 elementwise torch ops over all anchors, three device-to-host copies, NumPy argmax /
    back-projection / argsort, then the first 500 boxes to the NMS layer and the gather of the kept rows on the host"""
    means, stds = d["bbox_means"], d["bbox_stds"]
    rois = t["rois"]
    tracker = rois[:, 4].cpu().numpy().astype(np.int64)
    src = torch.from_numpy(d["anchors"][tracker, 4:]).cuda().float()
    p2_inv = np.linalg.inv(d["p2"])
    outs = []
    for b in range(t["prob"].shape[0]):
        b3 = t["bbox_3d"][b]
        x, y, z, w, h, l = [b3[:, i] * stds[0, 4 + i] + means[0, 4 + i] for i in range(6)]
        rsin = b3[:, 6] * stds[0, 11] + means[0, 11]
        rcos = b3[:, 7] * stds[0, 12] + means[0, 12]
        widths = rois[:, 2] - rois[:, 0] + 1.0
        heights = rois[:, 3] - rois[:, 1] + 1.0
        ctr_x = rois[:, 0] + 0.5 * widths
        ctr_y = rois[:, 1] + 0.5 * heights
        x = x * widths + ctr_x
        y = y * heights + ctr_y
        z = src[:, 0] + z
        w, h, l = torch.exp(w) * src[:, 1], torch.exp(h) * src[:, 2], torch.exp(l) * src[:, 3]
        rsin = src[:, 5] + rsin
        ry = src[:, 6] + rcos
        am, hm = b3[:, 8] >= 0.5, b3[:, 9] >= 0.5
        ry[am] = rsin[am]
        ry[hm] = ry[hm] + math.pi
        c3 = torch.stack((x, y, z, w, h, l, ry), dim=1)
        d2 = t["bbox_2d"][b] * torch.from_numpy(stds[0, :4]).cuda().float() + torch.from_numpy(means[0, :4]).cuda().float()
        pcx, pcy = d2[:, 0] * widths + ctr_x, d2[:, 1] * heights + ctr_y
        pw, ph = torch.exp(d2[:, 2]) * widths, torch.exp(d2[:, 3]) * heights
        c2 = torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1), dim=1)
        c2, c3, prob = c2.cpu().numpy(), c3.cpu().numpy(), t["prob"][b].cpu().numpy()
        acc = t["acceptance_prob"][b, :, 0].cpu().numpy()
        c2 /= sf
        c3[:, 0:2] /= sf
        cls = np.argmax(prob[:, 1:], axis=1) + 1
        scores = np.amax(prob[:, 1:], axis=1) * acc
        proj = p2_inv.dot(np.vstack((c3[:, 0] * c3[:, 2], c3[:, 1] * c3[:, 2], c3[:, 2], np.ones(len(c3)))))
        ry3d = c3[:, 6] + np.arctan2(-proj[2], proj[0]) + 0.5 * math.pi
        ry3d = (ry3d + math.pi) % (2 * math.pi) - math.pi
        raw = c3.copy()
        raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 6] = proj[0], proj[1], proj[2], ry3d
        order = (-scores).argsort()[:3000]
        ab = np.hstack((c2[order], scores[order, None]))[:500].astype(np.float32)
        out = G.differentiable_nms_with_iou2d_batched(torch.from_numpy(ab[None, :, 4]).cuda(), torch.from_numpy(ab[None, :, :4].copy()).cuda())
        n = counts_to_host(out[4], out[5])[0]
        keep = out[2][0, :n].cpu().numpy()
        rows = np.hstack((ab, cls[order][:500, None], c3[order][:500], tracker[order][:500, None]))[keep]
        rows[:, 0:4:2] = np.clip(rows[:, 0:4:2], 0, hw[1] - 1)
        rows[:, 1:4:2] = np.clip(rows[:, 1:4:2], 0, hw[0] - 1)
        outs.append(rows)
    return outs


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=["ours", "baseline"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B in (1, 2):
        d = synthetic.detection_heads(np.random.default_rng(11), B)
        sf, hw = 0.75, (683, 2347)
        t = {k: torch.from_numpy(d[k]).cuda() for k in ("prob", "bbox_2d", "bbox_3d", "rois")}
        t["anchors"] = torch.from_numpy(d["anchors"]).float().cuda()
        t["acceptance_prob"] = torch.from_numpy(d["acceptance"]).cuda()
        inv, sft, hwt = detect.camera_constants(d["p2"], sf, hw, B)

        def ours():
            det, counts = detect.detections_from_heads(t["prob"], t["bbox_2d"], t["bbox_3d"], t["rois"], t["anchors"], d["bbox_means"], d["bbox_stds"],
                                                       None, sft, hwt, t["acceptance_prob"], p2_inv=inv, clip_boxes=True)
            c = counts.tolist()                                           # what a caller that wants arrays pays: the counts and the rows
            return [det[b, :c[b]].cpu().numpy() for b in range(B)]
        rec = dict(tool="detect3d_time", B=B, A=int(d["rois"].shape[0]), nms_topN_pre=3000, groomed_topN=500, reps=a.reps)
        if a.only != "baseline":
            rec["ours_ms_median"], rec["ours_ms_min"] = median_ms(ours, a.reps)
        if a.only != "ours":
            rec["baseline_ms_median"], rec["baseline_ms_min"] = median_ms(lambda: baseline(t, d, sf, hw), max(5, a.reps // 5), warmup=2)
        if a.only is None:
            o, r = ours(), baseline(t, d, sf, hw)
            rec["same_kept_counts"] = [len(x) for x in o] == [len(x) for x in r]
            rec["kept"] = [len(x) for x in o]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
