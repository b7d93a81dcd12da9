"""Developer: the sorts alone per route (gnms_profile_sorts: 0 = what launch_sorts takes, 1 = runs + merge, 2 = ranked runs, 3 = by histogram),
20 calls captured in a HIP graph and replayed 30 times, us per call, median and minimum of the replays; two passes over the table.  Then the
cap series of the histogram sort: scores drawn from k distinct values fill bins of about N / k keys; route 3 with the fallback forced off
(cap 769) and forced on (cap 0).  `python tools/sort_routes.py [table] [cap]`"""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groomed_nms_amd import _lib, synthetic
from groomed_nms_amd._lib import GnmsParams, ptr, check, stream_ptr
lib = _lib.load()
P = GnmsParams(); lib.gnms_default_params(ctypes.byref(P))
CALLS, REPLAYS = 20, 30


def per_call_us(scores, boxes, route):
    B, N = scores.shape
    nbytes = lib.gnms_workspace_bytes(B, N, ctypes.byref(P))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        check(lib.gnms_profile_sorts(ptr(scores), ptr(boxes), B, N, None, route, None, None, None, None, None, None, None, ptr(ws), nbytes, stream_ptr()), "sorts")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            call()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / CALLS)
    del g
    return float(np.median(ts)), float(np.min(ts))


def table():
    print("B N boxes | route0 med/min | route1 (runs+merge) med/min | route2 (ranked runs) med/min | route3 (histogram) med/min  [us per call]", flush=True)
    shapes = ((1, 4096, 1), (2, 4096, 1), (4, 4096, 1), (8, 4096, 1), (16, 4096, 1), (8, 4096, 0), (16, 4096, 0), (32, 4096, 0), (8, 2112, 1), (8, 3072, 1))
    for _ in range(2):
        for B, N, wb in shapes:
            b, s = synthetic.batch_2d(1000, B, N, "uniform")
            scores, boxes = torch.from_numpy(s).cuda(), (torch.from_numpy(b).cuda() if wb else None)
            print("%2d %4d %d | %s" % (B, N, wb, " | ".join("%6.2f %6.2f" % per_call_us(scores, boxes, r) for r in (0, 1, 2, 3))), flush=True)
    for kind in ("clustered",):
        b, s = synthetic.batch_2d(1000, 8, 4096, kind)
        scores, boxes = torch.from_numpy(s).cuda(), torch.from_numpy(b).cuda()
        print("%s 8 4096 1 | %s" % (kind, " | ".join("%6.2f %6.2f" % per_call_us(scores, boxes, r) for r in (0, 1, 2, 3))), flush=True)


def cap_series():
    print("B N boxes | values k | largest number of equal scores | histogram forced (cap 769) med/min | fallback forced (cap 0) med/min  [us per call]", flush=True)
    rng = np.random.default_rng(13)
    for B, N, wb in ((8, 4096, 1), (8, 4096, 0)):
        b, _ = synthetic.batch_2d(1000, B, N, "uniform")
        boxes = torch.from_numpy(b).cuda() if wb else None
        for k in (1024, 512, 256, 128, 64, 48, 32, 24, 16, 12, 8, 6):
            s = ((rng.integers(0, k, size=(B, N)) + 0.5) / k).astype(np.float32)
            most = max(np.unique(s[i], return_counts=True)[1].max() for i in range(B))
            scores = torch.from_numpy(s).cuda()
            row = []
            for cap in (769, 0):
                lib.gnms_profile_set_hist_cap(cap)
                row.append("%6.2f %6.2f" % per_call_us(scores, boxes, 3))
            lib.gnms_profile_set_hist_cap(-1)
            print("%2d %4d %d | %4d | %4d | %s" % (B, N, wb, k, most, " | ".join(row)), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["table", "cap"]
    if "table" in what:
        table()
    if "cap" in what:
        cap_series()
