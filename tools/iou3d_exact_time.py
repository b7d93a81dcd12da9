"""Times the exact rotated IoU (gnms_iou3d_exact_from_params with iou_bev, csrc/iou3d_exact.hip) beside the yardstick that writes
the same 8 * B * N^2 bytes, gnms_iou3d_from_params(method 0) with iou_bev (the AABB approximation), with HIP events in one run.
Shapes: B = 1 / N = 500 (the reference's size), B = 8 / N = 4096, B = 1 / N = 16384 on uniform and clustered synthetic.boxes_3d,
and one adversarial set (4096 boxes jittered around a single centre: nearly every pair overlaps).
clipped = the fraction of pairs whose footprint AABBs overlap, i.e. the pairs the kernel clips.
usage: python tools/iou3d_exact_time.py [--iters K]  -> one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groomed_nms_amd import overlaps, synthetic, _lib  # noqa: E402


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def clipped_fraction(params):
    c = overlaps.corners_batched(params)[:, :, :, [7, 2, 3, 6]]           # footprints [B, N, 3, 4]
    x0, x1 = c[:, :, 0].amin(-1), c[:, :, 0].amax(-1)
    z0, z1 = c[:, :, 2].amin(-1), c[:, :, 2].amax(-1)
    hits = 0
    for b in range(params.shape[0]):
        for i in range(0, params.shape[1], 2048):
            sl = slice(i, i + 2048)
            ox = torch.maximum(x0[b, sl, None], x0[b, None]) < torch.minimum(x1[b, sl, None], x1[b, None])
            oz = torch.maximum(z0[b, sl, None], z0[b, None]) < torch.minimum(z1[b, sl, None], z1[b, None])
            hits += int((ox & oz).sum())
    return hits / (params.shape[0] * params.shape[1] ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    lib = _lib.load()
    rng = np.random.default_rng(0)
    sets = []
    for B, N in ((1, 500), (8, 4096), (1, 16384)):
        for clustered in (False, True):
            sets.append(("clustered" if clustered else "uniform", B, N,
                         np.stack([synthetic.boxes_3d(rng, N, clustered) for _ in range(B)])))
    p = synthetic.boxes_3d(rng, 4096)
    p[:, 0] = rng.normal(0, 0.3, 4096)
    p[:, 1] = 1.5 + rng.normal(0, 0.05, 4096)
    p[:, 2] = 30 + rng.normal(0, 0.3, 4096)
    sets.append(("one_centre", 1, 4096, p[None]))
    for kind, B, N, par in sets:
        a = torch.from_numpy(par.astype(np.float32)).cuda()
        bev = torch.empty((B, N, N), device="cuda")
        i3 = torch.empty((B, N, N), device="cuda")
        st = _lib.stream_ptr()

        def exact():
            _lib.check(lib.gnms_iou3d_exact_from_params(a.data_ptr(), a.data_ptr(), B, N, N, 0, bev.data_ptr(), i3.data_ptr(), N, st),
                       "gnms_iou3d_exact_from_params")

        def approx():
            _lib.check(lib.gnms_iou3d_from_params(a.data_ptr(), a.data_ptr(), B, N, N, 0, bev.data_ptr(), i3.data_ptr(), N, st),
                       "gnms_iou3d_from_params")

        iters = args.iters if N >= 4096 else 10 * args.iters
        t_exact = timed(exact, iters)
        t_approx = timed(approx, iters)
        t_exact2 = timed(exact, iters)                # again after the yardstick: both orders in the same run
        print(json.dumps({"boxes": kind, "B": B, "N": N, "exact_us": round(min(t_exact, t_exact2), 1),
                          "exact_us_runs": [round(t_exact, 1), round(t_exact2, 1)], "approx_method0_us": round(t_approx, 1),
                          "ratio": round(min(t_exact, t_exact2) / t_approx, 3),
                          "GB_per_s_exact": round(8.0 * B * N * N / min(t_exact, t_exact2) / 1e3, 1),
                          "clipped": round(clipped_fraction(a), 4)}), flush=True)


if __name__ == "__main__":
    main()
