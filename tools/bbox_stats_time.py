"""Times dataset_stats.compute_bbox_stats (gnms_gt_filter, gnms_compute_targets, gnms_bbox_stats_partials, gnms_bbox_stats_finish;
csrc/bbox_stats.hip) on a synthetic imdb of KITTI's training split's size: 3 712 images of five sizes with feat_size
32 x 106..110 at test_scale 512 and stride 16, about five ground truths each, the 36 anchors of 12 scales x 3 ratios (set by
generate_anchors on the same imdb, timed too: host NumPy).
Per batch size one child process under its own `timeout`; the child warms up on the first 64 images, then times whole calls with
cache_folder=None (wall clock around the call, device idle before and after): the record packing on the host, both passes and the one
read at the end.  The parent never touches the GPU, stops at the first child that fails and writes one JSON line per batch size.
There is no threshold and no earlier figure to compare with: the reference does this work on the host (7 424 NumPy compute_targets
calls) and nobody has timed that here.
usage: python tools/bbox_stats_time.py [--images N] [--batch-sizes 16,64] [--repeats K] [--limit S] [--out profiles/bbox_stats_time.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((375, 1242), (370, 1224), (374, 1260), (376, 1285), (375, 1285))      # -> feat_size 32 x 106, 106, 108, 110, 110


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def make_conf():
    scales = [float(32 * (512 / 32) ** (i / 11)) for i in range(12)]
    return AttrDict(anchor_scales=scales, anchor_ratios=[0.5, 1.0, 1.5], feat_stride=16, test_scale=512, has_3d=True, decomp_alpha=True,
                    lbls=["Car", "Pedestrian", "Cyclist"], ilbls=["Van", "Truck", "Person_sitting", "Tram", "Misc", "DontCare"],
                    min_gt_vis=0.65, min_gt_h=32.0, max_gt_h=10e10, fg_thresh=0.5, ign_thresh=0.5, bg_thresh_lo=0.0, bg_thresh_hi=0.5,
                    best_thresh=0.35)


def make_imdb(conf, n_images, seed=0):
    rng = np.random.default_rng(seed)
    shapes = [(s, r) for s in conf.anchor_scales for r in conf.anchor_ratios]
    imdb, k = [], 0
    for i in range(n_images):
        imH, imW = SIZES[i % len(SIZES)]
        sf = conf.test_scale / imH
        gts = []
        for _ in range(int(rng.integers(0, 11)) if i % 97 else 0):             # about five; some images have none
            hs, ratio = shapes[k % len(shapes)]
            k += 1
            h, w = hs * rng.uniform(0.95, 1.05) / sf, hs * ratio * rng.uniform(0.95, 1.05) / sf
            x, y = rng.uniform(0, max(imW - w, 1.0)), rng.uniform(0, max(imH - h, 1.0))
            b3 = np.zeros(16)
            b3[0:2] = (x + w / 2, y + h / 2)
            b3[2] = rng.uniform(3, 70)
            b3[3:6] = rng.uniform(0.5, 4.5, 3)
            b3[6], b3[11] = rng.uniform(-3.1, 3.1, 2)
            b3[12], b3[13] = np.sin(b3[11]), np.cos(b3[11])
            u = rng.random()
            gts.append(AttrDict(cls="Car" if u < 0.6 else "Pedestrian" if u < 0.75 else "Cyclist" if u < 0.85 else "Van" if u < 0.95 else "Other",
                                ign=False, visibility=1.0 if rng.random() < 0.85 else 0.3, trunc=0.0 if rng.random() < 0.85 else 0.7,
                                bbox_full=np.array([x, y, w, h]), bbox_3d=b3))
        imdb.append(AttrDict(gts=gts, scale=1.0, imH=imH, imW=imW))
    return imdb


def child(args):
    import torch
    from groomed_nms_amd import dataset_stats as D, _lib
    _lib.load()
    conf = make_conf()
    imdb = make_imdb(conf, args.images)
    t0 = time.perf_counter()
    D.generate_anchors(conf, imdb, None)
    t_anchors = time.perf_counter() - t0
    t0 = time.perf_counter()
    packed = D.pack_records(conf, imdb)
    t_pack = time.perf_counter() - t0
    batch = args.child
    D.compute_bbox_stats(conf, imdb[:64], None, batch_size=batch)                # warm-up: library, kernels, allocator
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        D.compute_bbox_stats(conf, imdb, None, batch_size=batch)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    means, stds = conf.bbox_means.copy(), conf.bbox_stds.copy()
    groups = D.group_by_feat_size(packed)
    print(json.dumps(dict(
        images=args.images, images_with_gts=int((packed.counts > 0).sum()), ground_truths=int(packed.counts.sum()), anchors=int(conf.anchors.shape[0]),
        feat_sizes={"%dx%d" % k: len(v) for k, v in groups.items()}, batch_size=batch, repeats=args.repeats,
        compute_bbox_stats_wall_s=dict(median=round(statistics.median(walls), 4), min=round(min(walls), 4), all=[round(w, 4) for w in walls]),
        of_which_pack_records_host_s=round(t_pack, 4), generate_anchors_host_s=round(t_anchors, 4),
        device=torch.cuda.get_device_name(0), bbox_means=means[0].tolist(), bbox_stds=stds[0].tolist(),
        peak_device_MB=round(torch.cuda.max_memory_allocated() / 1e6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3712)
    ap.add_argument("--batch-sizes", default="16,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbox_stats_time.jsonl"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    lines = []
    for batch in [int(b) for b in args.batch_sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(batch), "--images", str(args.images),
               "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                                    # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("the child for batch size %d ended with %d" % (batch, r.returncode))
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    same = {json.dumps([json.loads(ln)["bbox_means"], json.loads(ln)["bbox_stds"]]) for ln in lines}
    assert len(same) == 1, "the batch sizes disagree"
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
