"""Times heads.assemble_heads (gnms_heads_assemble, gnms_heads_assemble_backward, csrc/heads.hip) at the model's call
site: B = 2, A = 36, H = 32, W = 110, C = 4, i.e. R = 126 720 anchors per image, next to a stock-torch restatement of
models/densenet121_3d_dilate_decomp_alpha.py:166-215 (view, softmax, three sigmoids, fifteen permute-and-copy, two cat, a clone) on the
same device in the same process -- what a user of the reference runs today.
Four variants of each: forward eager, forward + backward eager (torch.autograd.grad w.r.t. all fifteen maps for five fixed cotangents),
and both replayed from a captured graph.  Per variant: HIP events around one call, median and minimum of --iters calls after a warm-up.
One graph is alive at a time.  The algorithmic bytes ((C + 14) floats read and (2C + 15) written per anchor forward, (2C + 15) + C + 3
read and (C + 14) written backward) over the replayed time are reported as a fraction of the 8 TB/s peak.  Before anything is timed the
two are compared at this size: the pure-layout outputs bit for bit, the others within 1e-5 (cotangents of up to five, a few
float32 roundings in another order).
GNMS_HEADS_ROW_STORES is read once per process, so the plain per-lane row stores are timed by a child process (--row-stores starts
one, after this process has finished its own timing, with the switch set and --no-torch); its figures join the line as row_stores_*.
The script ends itself after --limit seconds.
usage: python tools/heads_time.py [--iters K] [--out FILE] [--no-torch] [--row-stores]  -> one JSON line."""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import heads, _lib  # noqa: E402

B, A, H, W, C = 2, 36, 32, 110, 4
R = A * H * W
PEAK = 8.0e12
BYTES_F = B * R * ((C + 14) + (2 * C + 15)) * 4
BYTES_FB = BYTES_F + B * R * ((2 * C + 15) + C + 3 + (C + 14)) * 4


def median_us(fn, iters, warm=10):
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
    return round(statistics.median(ts), 2), round(min(ts), 2)


def flatten(t):
    """flatten_tensor (rpn_util.py:739): [B, c, A H, W] -> [B, A H W, c]"""
    return t.permute(0, 2, 3, 1).contiguous().view(t.shape[0], -1, t.shape[1])


def stock_torch(cls_map, box_maps, acceptance_map):
    """:166-215 with the reference's own sequence of operations; axis and head get their sigmoid on the map, as :162-163 do"""
    box = list(box_maps)
    box[11], box[12] = torch.sigmoid(box[11]), torch.sigmoid(box[12])
    cls = cls_map.view(B, C, H * A, W)
    prob = torch.softmax(cls, dim=1)
    col = [flatten(t.view(B, 1, H * A, W)) for t in box]
    bbox_2d = torch.cat(col[:4], dim=2)
    bbox_3d = torch.cat(col[4:11] + [col[10].clone(), col[11], col[12]], dim=2)
    cls, prob = flatten(cls), flatten(prob)
    acceptance = torch.sigmoid(flatten(acceptance_map.view(B, 1, H * A, W)))
    return cls, prob, bbox_2d, bbox_3d, acceptance


def replayed(step, iters, dev):
    """`step` captured into one graph on a side stream, replayed and timed; the graph is released before the next one is made"""
    step()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep = step()
    torch.cuda.synchronize()
    res = median_us(graph.replay, iters)
    torch.cuda.synchronize()
    del keep, graph
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the script ends itself")
    ap.add_argument("--no-torch", action="store_true", help="skip the stock-torch restatement")
    ap.add_argument("--row-stores", action="store_true", help="also time GNMS_HEADS_ROW_STORES=1 in a child process")
    args = ap.parse_args()
    signal.alarm(args.limit)
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    shapes = [(B, C * A, H, W)] + [(B, A, H, W)] * 14
    maps = [torch.from_numpy(rng.normal(0, 1.5, s).astype(np.float32)).to(dev).requires_grad_(True) for s in shapes]
    gs = [torch.from_numpy(rng.normal(0, 1, (B, R, c)).astype(np.float32)).to(dev) for c in (C, C, 4, 10, 1)]

    def ours():
        return heads.assemble_heads(maps[0], maps[1:14], maps[14])

    def stock():
        return stock_torch(maps[0], maps[1:14], maps[14])

    def forward(fn):
        def step():
            with torch.no_grad():
                return fn()
        return step

    def forward_backward(fn):
        def step():
            return torch.autograd.grad(list(fn()), maps, gs)
        return step

    line = dict(B=B, A=A, H=H, W=W, C=C, R=R, iters=args.iters, row_stores=os.environ.get("GNMS_HEADS_ROW_STORES", "0") == "1",
                MB_forward=round(BYTES_F / 1e6, 2), MB_forward_backward=round(BYTES_FB / 1e6, 2))
    variants = [("ours", ours)]
    if not args.no_torch:
        variants.append(("stock_torch", stock))
        got, want = forward(ours)(), forward(stock)()
        gg, gw = forward_backward(ours)(), forward_backward(stock)()
        torch.cuda.synchronize()
        assert all(torch.equal(got[i], want[i]) for i in (0, 2)) and torch.equal(got[3][:, :, :8], want[3][:, :, :8]), "layout outputs differ"
        line["max_difference_from_stock_torch"] = max(float((a - b).abs().max()) for a, b in list(zip(got, want)) + list(zip(gg, gw)))
        assert line["max_difference_from_stock_torch"] < 1e-5, line
        del got, want, gg, gw
    for name, fn in variants:
        for what, step, nbytes in (("forward", forward(fn), BYTES_F), ("forward_backward", forward_backward(fn), BYTES_FB)):
            line["%s_%s_us" % (name, what)], line["%s_%s_min_us" % (name, what)] = median_us(step, args.iters)
            us, mn = replayed(step, args.iters, dev)
            line["%s_%s_graph_us" % (name, what)], line["%s_%s_graph_min_us" % (name, what)] = us, mn
            if name == "ours":
                line["%s_graph_fraction_of_8TBs" % what] = round(nbytes / (us * 1e-6) / PEAK, 4)
    if not args.no_torch:
        for what in ("forward", "forward_backward", "forward_graph", "forward_backward_graph"):
            line["stock_torch_over_ours_" + what] = round(line["stock_torch_%s_us" % what] / line["ours_%s_us" % what], 2)
    torch.cuda.synchronize()
    if args.row_stores:
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--no-torch", "--iters", str(args.iters)],
                           env=dict(os.environ, GNMS_HEADS_ROW_STORES="1"), capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the row-stores child ended with %d: %s" % (r.returncode, r.stderr[-2000:]))
        child = json.loads(r.stdout.strip().splitlines()[-1])
        assert child["row_stores"]
        line.update({"row_stores_" + k[5:]: v for k, v in child.items() if k.startswith("ours_")})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
