"""Times the anchor sampler and the weighted classification term (gnms_sample_anchors, gnms_cls_loss, csrc/sampling.hip) at the loss's
call site: R = 32 * 110 * 36 = 126 720 anchors per image, C = 4, box_samples = fg_fraction = 0.2, about 1 % foreground and 3 %
ignore, B = 2 and 8.
Reports per shape: the device time of each call (HIP events around one call, the median of --iters steps after a warm-up), the same for
both calls replayed from one captured graph (no host work between the launches), the algorithmic bytes (sampler: R * (4 C + 4 + 24) per
image = prob and the label column read once, labels 8 + bbox_weights 4 + labels_scores 4 + sampled 1 + fg_index 4 + slack written; loss:
R * (8 C + 16) = cls read, dcls written, labels 8 + scores 4 read, labels_weight 4 written) as a fraction of 8 TB/s, and, for scale,
the NumPy restatement of tests/test_sampling_host.py for one image on the same host.
Per-kernel times: run this script under `rocprofv3 --kernel-trace --stats` (profiles/README.md).
usage: python tools/sampling_time.py [--iters K] [--out FILE]  -> one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from groomed_nms_amd import sampling, _lib  # noqa: E402
from test_sampling_host import restate      # noqa: E402  (the NumPy restatement the tests hold, timed for scale)

R, C = 126720, 4
PEAK = 8.0e12


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


def scene(rng, B):
    u = rng.random((B, R))
    t = -np.ones((B, R), np.float32)
    t[u < 0.01] = rng.integers(1, C, int((u < 0.01).sum()))
    t[(u >= 0.01) & (u < 0.04)] = 0
    cls = rng.normal(0, 2.0, (B, R, C)).astype(np.float32)
    prob = torch.softmax(torch.from_numpy(cls), dim=2).numpy()
    return t, prob, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    d = torch.device("cuda")
    kw = dict(box_samples=0.2, fg_fraction=0.2)
    lines = []
    for B in (2, 8):
        rng = np.random.default_rng(B)
        t, prob, cls = scene(rng, B)
        tt, pt, ct = (torch.from_numpy(a).to(d) for a in (t, prob, cls))
        vc = torch.ones(B, dtype=torch.int32, device=d)
        s = sampling.sample_anchors(tt, pt, vc, **kw)
        us_s, min_s = median_us(lambda: sampling.sample_anchors(tt, pt, vc, **kw), args.iters)
        us_l, min_l = median_us(lambda: sampling.classification_loss(ct, s, fg_fraction=0.2, focal_loss=0), args.iters)
        us_f, _ = median_us(lambda: sampling.classification_loss(ct, s, fg_fraction=0.2, focal_loss=2), args.iters)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s2 = sampling.sample_anchors(tt, pt, vc, **kw)
            sampling.classification_loss(ct, s2, fg_fraction=0.2, focal_loss=0)
        us_g, min_g = median_us(graph.replay, args.iters)
        b_s = B * R * (4 * C + 4 + 24)
        b_l = B * R * (8 * C + 16)
        line = dict(B=B, R=R, C=C, sample_anchors_us=round(us_s, 2), sample_anchors_min_us=round(min_s, 2),
                    cls_loss_us=round(us_l, 2), cls_loss_min_us=round(min_l, 2), cls_loss_focal2_us=round(us_f, 2),
                    both_graph_us=round(us_g, 2), both_graph_min_us=round(min_g, 2),
                    sampler_MB=round(b_s / 1e6, 2), loss_MB=round(b_l / 1e6, 2),
                    sampler_fraction_of_8TBs=round(b_s / (us_s * 1e-6) / PEAK, 4), loss_fraction_of_8TBs=round(b_l / (us_l * 1e-6) / PEAK, 4),
                    both_graph_fraction_of_8TBs=round((b_s + b_l) / (us_g * 1e-6) / PEAK, 4), iters=args.iters)
        if B == 2:
            t0 = time.perf_counter()
            restate(t[:1], prob[:1], np.array([1]), cls[:1], focal_loss=0, **kw)
            line["numpy_restatement_ms_per_image"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
