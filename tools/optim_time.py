"""Times the optimiser step (optim.FusedSGD, gnms_sgd_step, csrc/optim.hip) against the sequence it replaces, at the
parameter list of tools/e2e_bench.py's DenseNet121RPN (about 360 tensors, 12 M float32 parameters), in one process, alternating.

What is timed, per optimiser step:
  torch_*        torch.nn.utils.clip_grad_value_(params, 1) + torch.optim.SGD.step() + zero_grad(set_to_none=False), eager;
                 torch_gate_*: the same behind `if loss > 0:` as lib/core.py:102 has it (a host read of a device scalar)
  fused_*        FusedSGD.step(loss=loss), eager: one launch, the gate on the device
  *_graph_*      each captured in a graph and replayed (fused: capturable=True, the schedule on the device); the fused launch also with
                 non-temporal loads, stores or both, and with other grid sizes (workgroups per compute unit)
For each: *_cold_us = HIP events around ONE call that follows a sweep over --sweep-mib MiB (more than the 256 MiB Infinity Cache, so p,
g and buf come from HBM, as after a training step's backbone); *_warm_us = events around a burst of back-to-back calls, per call: the
144 MB of p + g + buf then stay in the Infinity Cache.  Eager figures are spans on the stream and include the gaps the host leaves
between launches; *_host_us is the host clock around the call without a synchronise (the enqueue).  Each is the median (and minimum)
of --iters repetitions after a warm-up.  identity_check_host_us: FusedSGD's per-step look at the addresses alone.
Also: the fused launch's bytes per second at 24 B per parameter, beside a plain float4 store stream (gnms_profile_fill) over the same
number of bytes timed the same way.  The script ends itself after --limit seconds.
usage: python tools/optim_time.py [--iters K] [--sweep-mib M] [--out FILE]  -> one JSON line."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from groomed_nms_amd import optim as O, _lib  # noqa: E402
from groomed_nms_amd._lib import check, ptr, stream_ptr  # noqa: E402
from e2e_bench import DenseNet121RPN  # noqa: E402

LR, MO, WD = 0.004, 0.9, 0.0005
BYTES_PER_PARAM = 24                                   # reads p, g, buf; writes p, buf and zeros into g


def med(ts, digits=1):
    return round(statistics.median(ts), digits), round(min(ts), digits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--sweep-mib", type=int, default=768)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="seconds after which the script ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    lib = _lib.load()
    assert torch.cuda.is_available(), "optim_time.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in DenseNet121RPN().parameters()]
    n_params = sum(int(np.prod(s)) for s in shapes)
    line = dict(tensors=len(shapes), parameters=n_params, MB_moved=round(n_params * BYTES_PER_PARAM / 1e6, 1), iters=args.iters,
                burst=args.burst, sweep_MiB=args.sweep_mib, chunk=O.CHUNK)
    sweep = torch.zeros((args.sweep_mib << 20) // 4, dtype=torch.float32, device=dev)
    loss = torch.tensor(1.5, device=dev)

    def make(n_sets):
        sets = []
        for _ in range(n_sets):
            ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.1) for s in shapes]
            for p in ps:
                p.grad = torch.randn_like(p) * 0.7
            sets.append(ps)
        return sets
    (pt, pf, pg, pc) = make(4)                         # torch eager, fused eager, torch graph, fused graph
    for dst in (pf, pg, pc):
        for a, b in zip(pt, dst):
            b.data.copy_(a.data)
            b.grad.copy_(a.grad)
    sgd = torch.optim.SGD(pt, lr=LR, momentum=MO, weight_decay=WD)
    sgd_g = torch.optim.SGD(pg, lr=LR, momentum=MO, weight_decay=WD)
    fused = O.FusedSGD(pf, lr=LR, momentum=MO, weight_decay=WD)
    table = np.full(1 << 16, LR, np.float64)
    fused_g = O.FusedSGD(pc, lr=LR, momentum=MO, weight_decay=WD, lr_table=table, capturable=True)

    def torch_seq(ps, opt):
        torch.nn.utils.clip_grad_value_(ps, 1)
        opt.step()
        opt.zero_grad(set_to_none=False)

    def torch_gate():
        if loss > 0:
            torch_seq(pt, sgd)

    # the same numbers first: one step of each from the same state, gradients included
    torch_seq(pt, sgd)
    fused.step(loss=loss)
    torch.cuda.synchronize()
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pt, pf))
    line["max_abs_difference_to_torch_after_one_step"] = worst
    assert worst <= 1e-7, "the fused step and torch's sequence differ by %g after one step" % worst
    assert all(not bool(p.grad.any()) for p in pf)
    line["fused_tasks"] = sum(g.n_tasks for g in fused._plans)

    def refill(ps):
        for p in ps:
            p.grad.normal_(0, 0.7)

    def cold(fn, ps=None):
        ts, hs = [], []
        for i in range(args.iters + 3):
            if ps is not None:
                refill(ps)
            sweep.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3)
                hs.append((t1 - t0) * 1e6)
        return ts, hs

    def warm(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.burst):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / args.burst)
        return ts

    def capture(fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.synchronize()
        return graph

    def report(name, fn, ps=None, host=True):
        ts, hs = cold(fn, ps)
        line[name + "_cold_us"], line[name + "_cold_min_us"] = med(ts)
        if host:
            line[name + "_host_us"], line[name + "_host_min_us"] = med(hs)
        line[name + "_warm_us"], line[name + "_warm_min_us"] = med(warm(fn))

    # eager, alternating
    report("torch", lambda: torch_seq(pt, sgd), pt)
    report("fused", lambda: fused.step(loss=loss), pf)
    report("torch_gate", torch_gate, pt)
    t = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        ok = fused._current()
        t.append((time.perf_counter() - t0) * 1e6)
    assert ok
    line["identity_check_host_us"], line["identity_check_host_min_us"] = med(t)

    # replayed
    try:
        g_torch = capture(lambda: torch_seq(pg, sgd_g))
        report("torch_graph", g_torch.replay, None, host=False)
    except Exception as e:                                                                # noqa: BLE001
        line["torch_graph_error"] = str(e)[:200]
        g_torch = None
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    graphs = {}
    for name, grid, nt in (("fused_graph", 0, 0), ("fused_graph_nt", 0, 3), ("fused_graph_nt_loads", 0, 1), ("fused_graph_nt_stores", 0, 2),
                           ("fused_graph_2_per_cu", 2 * cus, 0), ("fused_graph_8_per_cu", 8 * cus, 0)):
        O.GRID, O.NONTEMPORAL = grid, nt
        graphs[name] = capture(lambda: fused_g.step(loss=loss))
    O.GRID, O.NONTEMPORAL = 0, 0
    for _ in range(2):                                                                    # twice, alternating: the spread between equal runs
        for name, graph in graphs.items():
            key = name if name + "_cold_us" not in line else name + "_again"
            report(key, graph.replay, None, host=False)
    # a plain float4 store stream over as many bytes as the step moves, timed the same way
    sink = torch.empty((n_params * BYTES_PER_PARAM // 4,), dtype=torch.float32, device=dev)
    sp = stream_ptr(dev)
    report("fill", lambda: check(lib.gnms_profile_fill(ptr(sink), sink.numel(), sp), "fill"), None, host=False)
    moved = n_params * BYTES_PER_PARAM
    for k in ("fused_graph", "fused_graph_nt", "fill"):
        line[k + "_cold_TBs"] = round(moved / (line[k + "_cold_us"] * 1e-6) / 1e12, 3)
        line[k + "_warm_TBs"] = round(moved / (line[k + "_warm_us"] * 1e-6) / 1e12, 3)
    line["fused_graph_cold_rate_over_fill_cold"] = round(line["fill_cold_us"] / line["fused_graph_cold_us"], 3)
    if g_torch is not None:
        line["torch_graph_cold_over_fused_graph_cold"] = round(line["torch_graph_cold_us"] / line["fused_graph_cold_us"], 3)
    line["torch_cold_over_fused_cold"] = round(line["torch_cold_us"] / line["fused_cold_us"], 3)
    torch.cuda.synchronize()
    del graphs, g_torch
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
