"""Times the anchor target assignment (gnms_compute_targets, csrc/targets.hip) at the reference's configuration: R = 32 * 110 * 36 =
126 720 rois per image (crop 512 x 1760, stride 16, 36 anchors), float32 rois with rois_3d + centre, decomp_alpha, D3 = 16, the
call site's normalisation fused, B = 2 and 8, M in {12, 64, 256} ground truths and 4 ignore boxes per image.
Reports per shape: device time of compute_targets_batched without ols (HIP events), the algorithmic bytes (rois 20 + rois_3d 44 +
centre 8 read, transforms 92 + raw_gt 84 + ols_max 8 written = 256 B per roi) as a fraction of 8 TB/s, the NumPy drop-in
compute_targets end to end (host copies included, B = 1 image), and the NumPy checker of tests/test_targets_host.py for scale.
usage: python tools/targets_time.py [--iters K] [--out FILE]  -> one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from groomed_nms_amd import targets, _lib  # noqa: E402
from groomed_nms_amd.synthetic import anchor_scene  # noqa: E402
from test_targets_host import checker      # noqa: E402  (the NumPy restatement the tests hold, timed for scale)

TH = (0.5, 0.5, 0.0, 0.5, 0.35)            # fg, ign, bg_lo, bg_hi, best: scripts/config/groumd_nms.py

BYTES_PER_ROI = 20 + 44 + 8 + 92 + 84 + 8
PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    d = torch.device("cuda")
    lines = []
    for B in (2, 8):
        for M in (12, 64, 256):
            rng = np.random.default_rng(B * 1000 + M)
            s = anchor_scene(rng, B, Mmax=M, Kmax=4, garbage=False)
            s["Mc"][:] = M
            s["Kc"][:] = 4
            tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)      # noqa: E731
            ins = [tt(s[k]) for k in ("rois", "gv", "lb", "gi", "g3", "r3", "cen", "anchors")]
            means, stds = np.zeros(13), np.ones(13)
            ws_out = {}

            def call():
                r = targets.compute_targets_batched(ins[0], ins[1], ins[2], *TH, gts_ign=ins[3], gts_3d=ins[4], rois_3d=ins[5],
                                                    rois_3d_cen=ins[6], anchors=ins[7], means=means, stds=stds, out=ws_out)
                ws_out.update(transforms=r.transforms, raw_gt=r.raw_gt, ols_max=r.ols_max, best_roi=r.best_roi)
                return r
            us = timed(call, args.iters)
            R = s["rois"].shape[1]
            nbytes = BYTES_PER_ROI * B * R
            line = dict(B=B, R=R, M=M, K=4, device_us=round(us, 2), algorithmic_MB=round(nbytes / 1e6, 2),
                        fraction_of_8TBs=round(nbytes / (us * 1e-6) / PEAK, 3))
            if B == 2:
                b = 0
                kw = dict(gts_3d=s["g3"][b], anchors=s["anchors"], tracker=s["rois"][b][:, 4], rois_3d=s["r3"][b], rois_3d_cen=s["cen"][b])
                a = (s["gv"][b], s["gi"][b], s["lb"][b], s["rois"][b], *TH)
                targets.compute_targets(*a, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 5
                for _ in range(n):
                    targets.compute_targets(*a, **kw)
                line["drop_in_ms_per_image"] = round((time.perf_counter() - t0) / n * 1e3, 2)
                t0 = time.perf_counter()
                checker(*a, **kw)
                line["numpy_checker_ms_per_image"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
