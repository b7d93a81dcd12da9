"""Times the tail of a validation pass over a split: from the detections on the device to the float64 rows kitti_eval.evaluate takes.

  files   the file route, image by image: copy the kept boxes to the host, cut and threshold, kitti_io.convert_image_predictions_to_correct_entries,
          kitti_io.write_image_boxes_to_txt_file (one file per image), then kitti_eval.load_results over the folder and the upload
  device  kitti_results.KittiResults: append() per batch of 8 images, finish() (its one host read), device synchronise

Both routes start from the same detections_from_heads-shaped tensors (synthetic, seeded) and must end with the same rows (checked once,
exactly).  Host clock around work that ends in a device synchronise; one warm-up and several repetitions per route, alternating; the
result line gives the minimum, median and maximum of each.  Needs the GPU.

usage: python tools/validate_tail_bench.py [--images 3769] [--kmax 50] [--batch 8] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groomed_nms_amd import detect, kitti_eval, kitti_io  # noqa: E402
from groomed_nms_amd.kitti_results import KittiResults  # noqa: E402

LBLS = ["Car", "Pedestrian", "Cyclist"]
THRES, TOPN = 0.75, 50


def make_split(images, kmax, seed=0):
    rng = np.random.default_rng(seed)
    det = np.zeros((images, kmax, 14), np.float32)
    x1, y1 = rng.uniform(0, 1000, (images, kmax)), rng.uniform(0, 200, (images, kmax))
    det[..., 0], det[..., 1] = x1, y1
    det[..., 2], det[..., 3] = x1 + rng.uniform(20, 200, (images, kmax)), y1 + rng.uniform(20, 150, (images, kmax))
    det[..., 4] = -np.sort(-rng.uniform(0.5, 1.0, (images, kmax)), axis=1)                  # sorted, about half above the threshold
    det[..., 5] = rng.integers(1, 4, (images, kmax))
    det[..., 6], det[..., 7], det[..., 8] = rng.uniform(0, 1240, (images, kmax)), rng.uniform(120, 280, (images, kmax)), rng.uniform(5, 60, (images, kmax))
    det[..., 9], det[..., 10], det[..., 11] = rng.uniform(0.5, 2.0, (images, kmax)), rng.uniform(1.3, 2.0, (images, kmax)), rng.uniform(0.8, 4.5, (images, kmax))
    det[..., 12] = rng.uniform(-3.1, 3.1, (images, kmax))
    counts = rng.integers(0, kmax + 1, images).astype(np.int32)
    p2 = np.tile(np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.0027], [0, 0, 0, 1]]), (images, 1, 1))
    p2[:, 0, 2] += rng.uniform(-5, 5, images)
    return det, counts, p2


def files_route(det_d, counts_d, p2, folder):
    conf = dict(lbls=LBLS, score_thres=THRES, nms_topN_post=TOPN)
    data = os.path.join(folder, "data")
    os.makedirs(data)
    for b in range(det_d.shape[0]):
        n = int(counts_d[b])                                                                # im_detect_3d's host read
        aboxes = det_d[b, :n].cpu().numpy().astype(np.float64)
        aboxes = aboxes[:min(TOPN, aboxes.shape[0])]
        aboxes = aboxes[np.where(aboxes[:, 4] > THRES)[0]]
        boxes = kitti_io.convert_image_predictions_to_correct_entries(aboxes, conf, p2[b])
        kitti_io.write_image_boxes_to_txt_file(boxes, conf, data, "%06d" % b)
    rows, offsets, _ = kitti_eval.load_results(data)
    rows_d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    return rows_d, offsets


def device_route(det_d, counts_d, p2_inv, batch):
    images = det_d.shape[0]
    r = KittiResults(LBLS, THRES, TOPN, max_images=images, capacity_rows=images * TOPN)
    for b0 in range(0, images, batch):
        r.append(det_d[b0:b0 + batch], counts_d[b0:b0 + batch], p2_inv[b0:b0 + batch])
    rows_d, offsets = r.finish()
    torch.cuda.synchronize()
    return rows_d, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3769)
    ap.add_argument("--kmax", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("validate_tail_bench needs the GPU: a timing taken elsewhere says nothing")
    det, counts, p2 = make_split(a.images, a.kmax)
    det_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda()
    p2_inv = detect.camera_constants(p2, 1.0, (1, 1), a.images)[0]
    times = {"files": [], "device": []}
    root = tempfile.mkdtemp(prefix="validate_tail_")
    try:
        for rep in range(a.reps + 1):                                                       # repetition 0 is the warm-up
            t0 = time.perf_counter()
            rows_f, off_f = files_route(det_d, counts_d, p2, os.path.join(root, "rep%d" % rep))
            t1 = time.perf_counter()
            rows_n, off_n = device_route(det_d, counts_d, p2_inv, a.batch)
            t2 = time.perf_counter()
            if rep == 0:
                same = bool(off_f.tolist() == off_n.tolist() and torch.equal(rows_f, rows_n))
            else:
                times["files"].append(t1 - t0)
                times["device"].append(t2 - t1)
            shutil.rmtree(os.path.join(root, "rep%d" % rep))
    finally:
        shutil.rmtree(root, ignore_errors=True)

    def stats(v):
        return {"min_s": min(v), "median_s": float(np.median(v)), "max_s": max(v)}
    res = {"images": a.images, "kmax": a.kmax, "batch": a.batch, "reps": a.reps, "rows": int(off_n[-1]), "rows_identical": same,
           "files": stats(times["files"]), "device": stats(times["device"]),
           "speedup_median": float(np.median(times["files"]) / np.median(times["device"])), "gpu": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
