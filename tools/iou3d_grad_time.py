"""Times the cuboid gradient of the layer on the GPU, by the method of tools/iou_grad_time.py (whose measure / graphed /
backward_of it uses).  In one run, the variants alternating round by round:
  per shape (B = 2, N = 500 and the headline shape B = 8, N = 4096), the BACKWARD behind one gnms_forward_with_iou3d (default mode), C ABI:
    plain   gnms_backward without a matrix gradient: the backward a caller had before (the same launches as ever)
    sparse  gnms_backward_cuboids, default route: gnms_backward + bwd_masked_geometry_kernel<cuboids>
    dense   gnms_backward_cuboids, GNMS_BOXES_ROUTE_DENSE: gnms_backward with the matrix gradient + gnms_iou3d_backward (method 2)
  each eager (the ctypes call included) and replayed from a graph (the GPU's own time);
  gnms_iou3d_backward alone at B x N x N with a dense cotangent and with the masked layer's one-non-zero-per-row cotangent, beside
  gnms_profile_read over the same bytes and gnms_iou2d_backward on the same shape, on the same machine.
Device time by HIP events; per variant the median, minimum and the range of the rounds' medians (the run-to-run spread).
usage: python tools/iou3d_grad_time.py [--iters K] [--rounds N] [--out FILE]  -> one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from groomed_nms_amd import _lib, synthetic  # noqa: E402
from groomed_nms_amd._lib import check, ptr, stream_ptr  # noqa: E402
from iou_grad_time import backward_of, entry2, graphed, measure  # noqa: E402


def entry3(B, N, cot):
    lib = _lib.load()
    params = torch.from_numpy(synthetic.batch_3d(1, B, N, True, per=32)[0]).cuda()
    d = torch.empty((B, N, 7), device="cuda")
    ws = torch.empty((max(lib.gnms_iou3d_backward_workspace_bytes(B, N, N), 256),), dtype=torch.uint8, device="cuda")
    return lambda: check(lib.gnms_iou3d_backward(ptr(params), None, ptr(cot), B, N, N, N, 2, ptr(d), None, ptr(ws), ws.numel(), stream_ptr()),
                         "gnms_iou3d_backward")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    lines = []
    for B, N in ((2, 500), (8, 4096)):
        px, sc = synthetic.batch_3d(0, B, N, True, per=32)
        params, scores = torch.from_numpy(px).cuda(), torch.from_numpy(sc).cuda()
        eager = {v: backward_of(scores, params, v, "gnms_forward_with_iou3d", "gnms_backward_cuboids") for v in ("plain", "sparse", "dense")}
        res = dict(what="backward behind gnms_forward_with_iou3d, default mode", B=B, N=N, eager=measure(eager, a.iters, a.rounds))
        res["graph"] = measure({k: graphed(v) for k, v in eager.items()}, a.iters, a.rounds)
        lines.append(res)
    B, N = 8, 4096
    rng = np.random.default_rng(5)
    dense_cot = torch.from_numpy(rng.uniform(-1, 2, size=(B, N, N)).astype(np.float32)).cuda()
    sparse_cot = torch.zeros((B, N, N), device="cuda")
    rows = torch.arange(N, device="cuda")
    sparse_cot[:, rows, (rows * 7919) % N] = 1.0                      # one non-zero per row, as the masked layer's matrix gradient
    sink = torch.zeros(4096, device="cuda")
    read = lambda: check(lib.gnms_profile_read(ptr(dense_cot), dense_cot.numel(), ptr(sink), stream_ptr()), "gnms_profile_read")   # noqa: E731
    m = measure(dict(read=read, iou3d_backward_dense=entry3(B, N, dense_cot), iou3d_backward_one_per_row=entry3(B, N, sparse_cot),
                     iou2d_backward_dense=entry2(B, N, dense_cot), iou2d_backward_one_per_row=entry2(B, N, sparse_cot)), a.iters, a.rounds)
    nbytes = dense_cot.numel() * 4
    for k, v in m.items():
        v["TB_per_s_of_the_matrix"] = round(nbytes / (v["us_median"] * 1e-6) / 1e12, 3)
        v["share_of_read"] = round(m["read"]["us_median"] / v["us_median"], 3)
    lines.append(dict(what="gnms_iou3d_backward against gnms_profile_read over the same bytes and gnms_iou2d_backward on the same shape", B=B, N=N,
                      matrix_bytes=nbytes, **m))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
