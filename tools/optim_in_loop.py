"""Where the optimiser's time goes inside a whole eager training step: tools/e2e_bench.py's DenseNet121RPN on B = 4 images
of 512 x 1760 with a stand-in loss over its outputs, forward + backward + optimiser, for the four combinations of
{torch.optim.SGD, optim.FusedSGD} x {zero_grad(set_to_none=True), gradient tensors kept}, alternating, twice.  Per combination: ms per
step (host clock around 15 steps that end in a synchronise, after 4 warm-up steps) and how often FusedSGD rebuilt its device tables in
the timed steps.  usage: python tools/optim_in_loop.py [--out FILE]  -> one line per combination, then one JSON line."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from e2e_bench import DenseNet121RPN  # noqa: E402
from groomed_nms_amd import optim as O  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)
img = torch.randn((4, 3, 512, 1760), device=dev)
out = {}
calls = {"prepare": 0}
orig = O.FusedSGD.prepare
def counted(self):
    calls["prepare"] += 1
    return orig(self)
O.FusedSGD.prepare = counted

def run(kind, keep, steps=15, warm=4):
    net = DenseNet121RPN().to(dev)
    net.train()
    opt = O.FusedSGD(net.parameters(), lr=1e-4, momentum=0.9, clip_value=None) if kind == "fused" else torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)
    calls["prepare"] = 0
    def step():
        prob, d2, d3, _ = net(img)
        loss = prob.square().mean() + 1e-3 * (d2.square().mean() + d3.square().mean())
        if keep:
            opt.zero_grad(set_to_none=False) if kind == "torch" else opt.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        loss.backward()
        if kind == "fused":
            opt.step(loss=loss)
        else:
            opt.step()
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    before = calls["prepare"]
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return round(ms, 3), calls["prepare"] - before

for rnd in range(2):
    for kind, keep in (("torch", False), ("fused", False), ("torch", True), ("fused", True)):
        ms, rebuilt = run(kind, keep)
        out["%s_%s_%d" % (kind, "keep" if keep else "none", rnd)] = {"ms_per_step": ms, "tables_rebuilt_in_timed_steps": rebuilt}
        print(kind, keep, ms, rebuilt, flush=True)
print(json.dumps(out), flush=True)
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    with open(sys.argv[2], "w") as f:
        f.write(json.dumps(out) + "\n")
