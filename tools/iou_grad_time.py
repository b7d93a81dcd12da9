"""Times the box gradient of the layer on the GPU.  In one run, the variants alternating round by round:
  per shape (B = 2, N = 500 and the headline shape B = 8, N = 4096), the BACKWARD behind one gnms_forward_with_iou2d (default mode), C ABI:
    plain   gnms_backward without a matrix gradient: the backward a caller had before (the same launches as ever)
    sparse  gnms_backward_boxes, default route: gnms_backward + bwd_masked_geometry_kernel<boxes>
    dense   gnms_backward_boxes, GNMS_BOXES_ROUTE_DENSE: gnms_backward with the matrix gradient + gnms_iou2d_backward
  each eager (the ctypes call included) and replayed from a graph (the GPU's own time);
  gnms_iou2d_backward alone at B x N x N with a dense cotangent and with the masked layer's one-non-zero-per-row cotangent, beside
  gnms_profile_read over the same bytes on the same machine.
Device time by HIP events; per variant the median, minimum and the range of the rounds' medians (the run-to-run spread).
usage: python tools/iou_grad_time.py [--iters K] [--rounds N] [--out FILE]  -> one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import _lib, synthetic  # noqa: E402
from groomed_nms_amd import groomed_nms as GN  # noqa: E402
from groomed_nms_amd._lib import check, ptr, stream_ptr  # noqa: E402


def measure(variants, iters, rounds, warm=3):
    ts = {name: [] for name in variants}
    for fn in variants.values():
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
    for name, rs in ts.items():
        flat = [t for r in rs for t in r]
        med = [statistics.median(r) for r in rs]
        out[name] = dict(us_median=round(statistics.median(flat), 2), us_min=round(min(flat), 2),
                         us_round_medians=[round(min(med), 2), round(max(med), 2)])
    return out


def graphed(fn):
    fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.synchronize()
    return g.replay


def backward_of(scores, src, variant, forward="gnms_forward_with_iou2d", backward="gnms_backward_boxes"):
    """one `forward` (gnms_forward_with_iou2d on boxes, gnms_forward_with_iou3d on cuboids: tools/iou3d_grad_time.py) through the C ABI, then
    a closure that runs the backward alone on its workspace: plain = gnms_backward (no matrix gradient), sparse / dense = `backward`
    (gnms_backward_boxes / gnms_backward_cuboids) on that route"""
    import ctypes
    lib = _lib.load()
    B, N = scores.shape
    p = GN._params(0.4, "linear", 0.01, 0.3, False, True, True, 100, False, False)
    prob, order, _, _, nv, ni = GN._outputs(B, N, scores.device, False)
    matrix = torch.empty((B, N, N), device="cuda")
    ws = torch.empty((max(lib.gnms_workspace_bytes(B, N, ctypes.byref(p)), 256),), dtype=torch.uint8, device="cuda")
    check(getattr(lib, forward)(ptr(src), ptr(scores), B, N, N, None, ctypes.byref(p), ptr(matrix), ptr(prob), ptr(order), None, None,
                                ptr(nv), ptr(ni), ptr(ws), ws.numel(), stream_ptr()), forward)
    gp = torch.linspace(-1, 2, N, device="cuda").repeat(B, 1).contiguous()
    gs, gb = torch.empty_like(scores), torch.empty_like(src)
    if variant == "plain":
        return lambda: check(lib.gnms_backward(ptr(gp), ptr(scores), ptr(scores), B, N, N, None, ctypes.byref(p), ptr(gs), None, ptr(ws),
                                               ws.numel(), stream_ptr()), "gnms_backward")
    route = 1 if variant == "dense" else 0
    nb = getattr(lib, backward + "_scratch_bytes")(B, N, N, ctypes.byref(p), 1, route)
    scratch = torch.empty((max(nb, 256),), dtype=torch.uint8, device="cuda")
    return lambda: check(getattr(lib, backward)(ptr(gp), ptr(src), ptr(scores), B, N, None, ctypes.byref(p), ptr(gs), ptr(gb), ptr(matrix), N,
                                                route, ptr(scratch), nb, ptr(ws), ws.numel(), stream_ptr()), backward)


def entry2(B, N, cot):
    lib = _lib.load()
    boxes = torch.from_numpy(synthetic.batch_2d(1, B, N, "clustered", per=32)[0]).cuda()
    d = torch.empty((B, N, 4), device="cuda")
    ws = torch.empty((max(lib.gnms_iou2d_backward_workspace_bytes(B, N, N), 256),), dtype=torch.uint8, device="cuda")
    return lambda: check(lib.gnms_iou2d_backward(ptr(boxes), None, ptr(cot), B, N, N, N, ptr(d), None, ptr(ws), ws.numel(), stream_ptr()),
                         "gnms_iou2d_backward")


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
        bx, sc = synthetic.batch_2d(0, B, N, "clustered", per=32)
        boxes, scores = torch.from_numpy(bx).cuda(), torch.from_numpy(sc).cuda()
        eager = {v: backward_of(scores, boxes, v) for v in ("plain", "sparse", "dense")}
        res = dict(what="backward behind gnms_forward_with_iou2d, default mode", B=B, N=N, eager=measure(eager, a.iters, a.rounds))
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
    m = measure(dict(read=read, iou2d_backward_dense=entry2(B, N, dense_cot), iou2d_backward_one_per_row=entry2(B, N, sparse_cot)), a.iters, a.rounds)
    nbytes = dense_cot.numel() * 4
    for k, v in m.items():
        v["TB_per_s_of_the_matrix"] = round(nbytes / (v["us_median"] * 1e-6) / 1e12, 3)
        v["share_of_read"] = round(m["read"]["us_median"] / v["us_median"], 3)
    lines.append(dict(what="gnms_iou2d_backward against gnms_profile_read over the same bytes", B=B, N=N, matrix_bytes=nbytes, **m))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
