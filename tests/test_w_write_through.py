"""Write-through stores for the rows of W out of the LDS row buffer (w_rows_write_through, round 9: bitmask_boxes_kernel's row-buffer routes,
bitmask_kernel's 16-wave route), where plain stores left 16.8 MB dirty in L2 for the end-of-kernel release.  The switch is read once per
process, so every form runs in a fresh child:

    default        the library as it ships (the routes of kWtDefaultRoutes write through)
    plain          GNMS_W_WRITE_THROUGH=0: plain 8-byte stores on every route
    through        GNMS_W_WRITE_THROUGH=15: every row-buffer route written through, the chunk loop included

A child drives the C ABI through ctypes with a caller-owned workspace (as bench.py's raw_step does): gnms_forward_with_iou2d + gnms_backward on
one ragged batch per shape, once on a workspace full of 0x00 and once full of 0xFF -- a word of W the write-out skips or puts in the wrong
place then differs between the two.  In the child, bit for bit: the two fills; the matrix-in route (gnms_forward + gnms_backward) on the
matrix the call wrote; the whole matrix against gnms_iou2d of the same boxes (the launch that reads W also writes the matrix).  Here, bit
for bit: the three children; and the default child against the CPU oracle (index sets at tolerance 0, values at the project's 1e-4).  One
case also runs captured into a graph, three replays.

Shapes (B, N), the smallest at which each copy loop can go wrong:
    (8, 2112)  two rank blocks per workgroup with 33 rank blocks: the image's last workgroup has ONE row; a row is 16896 bytes, no multiple
               of the 16 KiB that 1024 lanes cover per pass
    (8, 2048)  one rank block per workgroup, the ranks stashed in LDS
    (4, 4096)  one rank block per workgroup at full width
    (8, 4096)  the headline's kernel
    (8, 2052)  NC = 2052: rows of 16416 bytes; N % 8 != 0 sends the matrix writers down their general path beside the packed one
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((8, 2112), (8, 2048), (4, 4096), (8, 4096), (8, 2052))
NAMES = ("prob", "order", "valid", "invalid", "nvalid", "ninvalid", "grad")
CHILDREN = (("default", {}),
            ("plain", {"GNMS_W_WRITE_THROUGH": "0"}),
            ("through", {"GNMS_W_WRITE_THROUGH": "15"}))


def ragged_counts(B, N):
    """0; 1; 65 and 1025 (n % 64 == 1, whole trailing rank blocks empty); N - 63 (n % 64 == 1 where 64 | N); full images."""
    return np.array([N, 0, 1, 1025, 65, N - 63, N - 1, N][:B] if B == 8 else [N, 0, 1, 1025], np.int32)


def inputs(B, N):
    from groomed_nms_amd import synthetic
    return synthetic.batch_2d(900 + N + B, B, N, "uniform" if N % 8 else "clustered")


_CHILD = r"""
import ctypes, importlib.util, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[2])
from groomed_nms_amd import _lib
from groomed_nms_amd._lib import GnmsParams, check, ptr, stream_ptr
spec = importlib.util.spec_from_file_location("w_write_through_cases", sys.argv[3])     # the shapes, counts and inputs of this file
cases = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cases)
SHAPES, NAMES, ragged_counts, inputs = cases.SHAPES, cases.NAMES, cases.ragged_counts, cases.inputs
lib = _lib.load()
dev = torch.device("cuda")
P = GnmsParams()
lib.gnms_default_params(ctypes.byref(P))
out = {}

class Case:
    def __init__(self, B, N):
        self.B, self.N = B, N
        b, s = inputs(B, N)
        self.boxes, self.scores = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
        self.counts = torch.from_numpy(ragged_counts(B, N)).to(dev)
        self.w = torch.linspace(-1.0, 2.0, N, device=dev).repeat(B, 1).contiguous()
        self.ws = torch.empty(lib.gnms_workspace_bytes(B, N, ctypes.byref(P)), dtype=torch.uint8, device=dev)
        self.iou = torch.empty((B, N, N), dtype=torch.float32, device=dev)
        self.o = dict(prob=torch.empty((B, N), device=dev), order=torch.empty((B, N), dtype=torch.int64, device=dev),
                      valid=torch.empty((B, N), dtype=torch.int64, device=dev), invalid=torch.empty((B, N), dtype=torch.int64, device=dev),
                      nvalid=torch.empty((B,), dtype=torch.int32, device=dev), ninvalid=torch.empty((B,), dtype=torch.int32, device=dev),
                      grad=torch.empty((B, N), device=dev))
    def poison(self):
        self.iou.view(torch.int32).fill_(0x7fc12345)                  # a NaN no kernel computes
        for k, v in self.o.items():
            v.fill_(-7)
    def forward(self, with_boxes):
        o, B, N, sp = self.o, self.B, self.N, stream_ptr(dev)
        if with_boxes:
            check(lib.gnms_forward_with_iou2d(ptr(self.boxes), ptr(self.scores), B, N, N, ptr(self.counts), ctypes.byref(P), ptr(self.iou),
                                              ptr(o["prob"]), ptr(o["order"]), ptr(o["valid"]), ptr(o["invalid"]), ptr(o["nvalid"]),
                                              ptr(o["ninvalid"]), ptr(self.ws), self.ws.numel(), sp), "gnms_forward_with_iou2d")
        else:
            check(lib.gnms_forward(ptr(self.scores), ptr(self.iou), B, N, N, ptr(self.counts), ctypes.byref(P), ptr(o["prob"]), ptr(o["order"]),
                                   ptr(o["valid"]), ptr(o["invalid"]), ptr(o["nvalid"]), ptr(o["ninvalid"]), ptr(self.ws), self.ws.numel(), sp),
                  "gnms_forward")
        check(lib.gnms_backward(ptr(self.w), ptr(self.scores), ptr(self.iou), B, N, N, ptr(self.counts), ctypes.byref(P), ptr(o["grad"]), None,
                                ptr(self.ws), self.ws.numel(), sp), "gnms_backward")
    def result(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.o.items()}

def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t

def same(a, b, what):
    for k in NAMES:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)

for B, N in SHAPES:
    c = Case(B, N)
    res = []
    for fill in (0x00, 0xFF):
        c.ws.fill_(fill)
        c.poison()
        c.forward(True)
        res.append(c.result())
    same(res[0], res[1], (B, N, "workspace fill"))
    # the whole matrix against gnms_iou2d of the same boxes, bit for bit (the rows of images past their count included: the writers know no counts)
    ref = torch.empty_like(c.iou)
    ref.view(torch.int32).fill_(0x7fc54321)
    check(lib.gnms_iou2d(ptr(c.boxes), ptr(c.boxes), B, N, N, ptr(ref), N, stream_ptr(dev)), "gnms_iou2d")
    torch.cuda.synchronize()
    assert torch.equal(c.iou.view(torch.int32), ref.view(torch.int32)), (B, N, "matrix")
    iv = c.iou.view(torch.int32)
    out["%d_%d_matrix_sums" % (B, N)] = np.array([int(iv.to(torch.int64).sum()), int((iv[:, ::7, :].to(torch.int64) * 3 + iv[:, ::7, :].to(torch.int64) // 5).sum()),
                                                   int(torch.isnan(c.iou).sum())], np.int64)
    out["%d_%d_matrix_row" % (B, N)] = c.iou[B - 1, N - 1].cpu().numpy()
    del ref, iv
    # the matrix-in route on the matrix the call wrote
    for fill in (0x00, 0xFF):
        c.ws.fill_(fill)
        for k, v in c.o.items():
            v.fill_(-7)
        c.forward(False)
        same(res[0], c.result(), (B, N, "matrix-in route", fill))
    for k in NAMES:
        out["%d_%d_%s" % (B, N, k)] = res[0][k].cpu().numpy()
    if (B, N) == (8, 2112):                                           # captured, three replays (default queue count: the graph has branches)
        c.ws.fill_(0xFF)
        c.forward(True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.forward(True)
        for rep in range(3):
            c.poison()
            g.replay()
            same(res[0], c.result(), (B, N, "replay", rep))
            assert torch.equal(c.iou[B - 1, N - 1].view(torch.int32).cpu(), torch.from_numpy(out["%d_%d_matrix_row" % (B, N)]).view(torch.int32)), (B, N, "replay", rep)
        del g
    del c
    torch.cuda.empty_cache()
np.savez(sys.argv[1], **out)
print("ok")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The three children, one after the other; their results are shared by the tests below and left unchanged."""
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    d = tmp_path_factory.mktemp("w_write_through")
    got = {}
    for tag, env in CHILDREN:
        path = str(d / ("%s.npz" % tag))
        e = dict(os.environ, **env)
        if not env:
            e.pop("GNMS_W_WRITE_THROUGH", None)
        r = subprocess.run([sys.executable, "-c", _CHILD, path, ROOT, os.path.abspath(__file__)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, (tag, r.stdout[-500:], r.stderr[-3000:])
        got[tag] = dict(np.load(path))
    return got


def test_children_agree_bit_for_bit(runs):
    """Outputs, gradient, and the matrix (two sums over its bit patterns, its NaN count and its last row) of the three forms."""
    d = runs["default"]
    assert len(d) == len(SHAPES) * (len(NAMES) + 2)
    for tag in ("plain", "through"):
        assert sorted(runs[tag]) == sorted(d)
        for k in d:
            assert d[k].tobytes() == runs[tag][k].tobytes(), (tag, k)


@pytest.mark.parametrize("B,N", SHAPES)
def test_default_against_the_oracle(runs, B, N):
    """Images 2 (one box), 3 (1025 boxes) and, up to N = 2112, the full image 0: index sets exactly, values within 1e-4."""
    from oracle import oracle as O
    d = {k: runs["default"]["%d_%d_%s" % (B, N, k)] for k in NAMES}
    boxes, scores = inputs(B, N)
    counts = ragged_counts(B, N)
    w = np.linspace(-1.0, 2.0, N).astype(np.float32)
    assert d["nvalid"][1] == 0 and d["ninvalid"][1] == 0                 # the image without boxes
    for b in (2, 3) + ((0,) if N <= 2112 else ()):
        n = int(counts[b])
        m = O.iou2d(boxes[b, :n], boxes[b, :n])
        ref = O.differentiable_nms(scores[b, :n], m, grad_prob=w[:n])
        assert d["order"][b, :n].tolist() == ref["order"].tolist(), (b, "order")
        assert d["valid"][b, :int(d["nvalid"][b])].tolist() == list(ref["valid"]), (b, "valid")
        assert sorted(d["invalid"][b, :int(d["ninvalid"][b])].tolist()) == sorted(ref["invalid"].tolist()), (b, "invalid")
        assert int(d["nvalid"][b]) + int(d["ninvalid"][b]) == n, (b, "counts")
        assert float(np.abs(d["prob"][b, :n] - ref["prob"]).max()) <= 1e-4, (b, "prob")
        assert float(np.abs(d["grad"][b, :n] - ref["grad_scores"]).max()) <= 1e-4, (b, "grad_scores")
    last = O.iou2d(boxes[B - 1, N - 1:N], boxes[B - 1])[0]
    assert runs["default"]["%d_%d_matrix_row" % (B, N)].tobytes() == last.astype(np.float32).tobytes(), "matrix row"
    assert int(runs["default"]["%d_%d_matrix_sums" % (B, N)][2]) == 0, "a word of the matrix was never written"
