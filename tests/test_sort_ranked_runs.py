"""The one-launch sort of 2048 < N <= 4096 keys per image (sort_ranked_runs_kernel: sixteen wave-sorted runs per workgroup, ranked in the
same launch) against the two-launch runs + merge it replaces.  Everything goes through gnms_profile_sorts in one process: route 2 against
route 1 bit for bit on every array the sorts leave behind and on both flags, and on plain inputs against NumPy's stable sorts.  The keys are
distinct (the index is in the low bits), so the order is unique and the two routes have nothing to differ in."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARRAYS = ("order", "rankof", "sscore", "rbox", "xidx", "xbox", "flags")
# (B, N): one real key in run 8 and runs 9-15 all padding; 2112; one key short of full; full; 288 workgroups with boxes (more than one round)
SHAPES = ((3, 2049), (3, 2112), (3, 4095), (3, 4096), (9, 2304))


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import _lib
    assert torch.cuda.is_available(), "these tests need the GPU"
    return _lib.load()


def _counts(B, N):
    """No counts, and the three ragged triples (repeated over the batch where B > 3)."""
    out = [None]
    for c in ([N, 0, 1], [64, 65, 1025], [N - 1, 256, 257]):
        out.append(np.array((c * ((B + 2) // 3))[:B], np.int32))
    return out


def _ns(counts, B, N):
    return [N] * B if counts is None else [int(c) for c in counts]


def _workspace(lib, B, N, fill=None):
    from groomed_nms_amd._lib import GnmsParams
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    ws = torch.empty(lib.gnms_workspace_bytes(B, N, ctypes.byref(P)), dtype=torch.uint8, device="cuda")
    ws.fill_(0 if fill is None else fill)
    return ws


def _sorts(lib, scores, boxes, counts, route, ws=None):
    from groomed_nms_amd._lib import check, ptr, stream_ptr
    B, N = scores.shape
    dev = torch.device("cuda")
    st = torch.from_numpy(scores).to(dev)
    bt = torch.from_numpy(boxes).to(dev) if boxes is not None else None
    ct = torch.from_numpy(counts).to(dev) if counts is not None else None
    if ws is None:
        ws = _workspace(lib, B, N)
    o = dict(order=torch.full((B, N), -7, dtype=torch.int32, device=dev), rankof=torch.full((B, N), -7, dtype=torch.int32, device=dev),
             sscore=torch.full((B, N), -7.0, device=dev), rbox=torch.full((B, N, 4), -7.0, device=dev),
             xidx=torch.full((B, N), -7, dtype=torch.int32, device=dev), xbox=torch.full((B, N, 4), -7.0, device=dev),
             flags=torch.full((B, 2), -7, dtype=torch.int32, device=dev))
    check(lib.gnms_profile_sorts(ptr(st), ptr(bt), B, N, ptr(ct), route, ptr(o["order"]), ptr(o["rankof"]), ptr(o["sscore"]), ptr(o["rbox"]),
                                 ptr(o["xidx"]), ptr(o["xbox"]), ptr(o["flags"]), ptr(ws), ws.numel(), stream_ptr()), "gnms_profile_sorts")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same(a, b, what):
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _both(lib, scores, boxes, counts, what):
    """Route 2 against route 1, bit for bit; returns the ranked-runs result."""
    one = _sorts(lib, scores, boxes, counts, 1)
    two = _sorts(lib, scores, boxes, counts, 2)
    _same(two, one, what)
    return two


def _plain(b):
    """box_orders_plainly: finite coordinates, no negative zero, x2 >= x1, y2 >= y1"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(b).all(-1) & ~((b == 0) & np.signbit(b)).any(-1) & (b[..., 2] >= b[..., 0]) & (b[..., 3] >= b[..., 1])


def _check_numpy(res, scores, boxes, counts, what, check_order=True):
    """The result against NumPy: stable descending argsort of the scores, stable ascending argsort of the x centres, padding, flags."""
    B, N = scores.shape
    for b, n in enumerate(_ns(counts, B, N)):
        s = scores[b, :n]
        if check_order:
            ref = np.argsort(-s, kind="stable")
            assert np.array_equal(res["order"][b, :n], ref), (what, b, "order")
            assert np.array_equal(res["sscore"][b, :n], s[ref]), (what, b, "sscore")
            assert res["flags"][b, 0] == int(np.all(s[:-1] >= s[1:])), (what, b, "sorted flag")
        assert np.array_equal(res["order"][b, n:], np.arange(n, N)), (what, b, "padding order")
        assert np.array_equal(res["rankof"][b, res["order"][b]], np.arange(N)), (what, b, "rankof")
        assert not res["sscore"][b, n:].any(), (what, b, "padding sscore")
        if boxes is None:
            assert res["flags"][b, 1] == 0 and not res["xidx"][b].any() and not res["rbox"][b].any()
            continue
        bx = boxes[b, :n]
        assert res["rbox"][b, :n].tobytes() == bx[res["order"][b, :n]].tobytes(), (what, b, "rbox")
        xref = np.argsort(bx[:, 0] + bx[:, 2], kind="stable")
        assert np.array_equal(res["xidx"][b, :n], xref), (what, b, "xidx")
        assert res["xbox"][b, :n].tobytes() == bx[xref].tobytes(), (what, b, "xbox")
        assert res["flags"][b, 1] == int(not _plain(bx).all()), (what, b, "plain flag")


def _scores(rng, B, N):
    from groomed_nms_amd import synthetic
    return np.stack([synthetic.tie_free_scores(rng, N) for _ in range(B)])


def _uniform(rng, B, N):
    from groomed_nms_amd import synthetic
    return np.stack([synthetic.uniform_boxes_2d(rng, N) for _ in range(B)])


@pytest.mark.parametrize("B,N", SHAPES)
def test_scores(lib, B, N):
    rng = np.random.default_rng(1000 + N)
    boxes = _uniform(rng, B, N)
    rnd = _scores(rng, B, N)
    desc = -np.sort(-rnd, axis=1)
    for counts in _counts(B, N):
        ns = _ns(counts, B, N)
        tag = (B, N, None if counts is None else counts[:3].tolist())
        _check_numpy(_both(lib, rnd, boxes, counts, tag + ("random",)), rnd, boxes, counts, tag + ("random",))
        res = _both(lib, desc, boxes, counts, tag + ("descending",))
        _check_numpy(res, desc, boxes, counts, tag + ("descending",))
        assert (res["flags"][:, 0] == 1).all(), tag
        for where in ("front", "run edge", "back"):                      # descending except for one swap
            sw = desc.copy()
            hit = []
            for b, n in enumerate(ns):
                i = {"front": 0, "run edge": 255, "back": n - 2}[where]
                if 0 <= i and i + 1 < n:
                    sw[b, [i, i + 1]] = sw[b, [i + 1, i]]
                    hit.append(b)
            res = _both(lib, sw, boxes, counts, tag + (where,))
            _check_numpy(res, sw, boxes, counts, tag + (where,))
            assert (res["flags"][np.array(hit, dtype=int), 0] == 0).all(), tag + (where,)
        equal = np.full((B, N), 0.5, np.float32)
        res = _both(lib, equal, boxes, counts, tag + ("equal",))
        _check_numpy(res, equal, boxes, counts, tag + ("equal",))
        assert np.array_equal(res["order"], np.tile(np.arange(N, dtype=np.int32), (B, 1))) and (res["flags"][:, 0] == 1).all(), tag
        eight = (rng.integers(0, 8, size=(B, N)) / 8.0).astype(np.float32)   # stable among ties
        _check_numpy(_both(lib, eight, boxes, counts, tag + ("eight values",)), eight, boxes, counts, tag + ("eight values",))
        special = rnd.copy()                                             # against runs + merge only
        pick = rng.integers(0, 6, size=(B, N))
        for v, val in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):
            special[pick == v] = val
        res = _both(lib, special, boxes, counts, tag + ("special",))
        _check_numpy(res, special, boxes, counts, tag + ("special",), check_order=False)


@pytest.mark.parametrize("B,N", SHAPES)
def test_boxes(lib, B, N):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(2000 + N)
    scores = _scores(rng, B, N)
    uniform = _uniform(rng, B, N)
    clustered = np.stack([synthetic.clustered_boxes_2d(rng, N, 32) for _ in range(B)]).astype(np.float32)
    blocks = uniform.copy()                                              # equal x centres in blocks of 300: ties go by index
    cx = np.repeat(rng.permutation((N + 299) // 300), 300)[:N].astype(np.float32) * 8.0
    blocks[:, :, 0], blocks[:, :, 2] = cx - 4.0, cx + 4.0
    nanx = uniform.copy()                                                # NaN x: these sort last
    nanx[:, rng.choice(N, 40, replace=False), 0] = np.nan
    for counts in _counts(B, N):
        ns = _ns(counts, B, N)
        tag = (B, N, None if counts is None else counts[:3].tolist())
        for name, bx in (("uniform", uniform), ("clustered", clustered), ("blocks", blocks), ("nan x", nanx)):
            res = _both(lib, scores, bx, counts, tag + (name,))
            _check_numpy(res, scores, bx, counts, tag + (name,))
            if name in ("uniform", "clustered", "blocks"):
                assert (res["flags"][:, 1] == 0).all(), tag + (name,)     # no box that is not plain
        for kind in ("x2 < x1", "nan", "minus zero"):                    # ONE box that is not plain, per image
            for where in ("run 0", "run 15", "last"):
                bx = uniform.copy()
                hit = []
                for b, n in enumerate(ns):
                    i = {"run 0": 7, "run 15": 15 * 256 + 7, "last": n - 1}[where]
                    if 0 <= i < n:
                        if kind == "x2 < x1":
                            bx[b, i, 2] = bx[b, i, 0] - 1.0
                        elif kind == "nan":
                            bx[b, i, 3] = np.nan
                        else:
                            bx[b, i, 1] = -0.0
                        hit.append(b)
                res = _both(lib, scores, bx, counts, tag + (kind, where))
                _check_numpy(res, scores, bx, counts, tag + (kind, where))
                assert (res["flags"][np.array(hit, dtype=int), 1] == 1).all(), tag + (kind, where)


@pytest.mark.parametrize("B,N", SHAPES + ((8, 4096), (32, 4096)))
def test_scores_alone(lib, B, N):
    """boxes = NULL: the matrix-in layer's sort, one role."""
    rng = np.random.default_rng(3000 + N + B)
    scores = _scores(rng, B, N)
    for counts in _counts(B, N):
        tag = (B, N, None if counts is None else counts[:3].tolist())
        _check_numpy(_both(lib, scores, None, counts, tag), scores, None, counts, tag)


def test_default_route_is_the_table(lib):
    """Route 0 is what the layer takes: ranked runs where the counting sort does not apply, and in either case the same arrays."""
    rng = np.random.default_rng(5)
    for B, N in ((1, 4096), (3, 2112), (8, 4096), (16, 4096)):         # counting, ranked runs twice, two rounds: runs + merge
        scores, boxes = _scores(rng, B, N), _uniform(rng, B, N)
        _same(_sorts(lib, scores, boxes, None, 0), _sorts(lib, scores, boxes, None, 1), (B, N))
    from groomed_nms_amd._lib import GnmsError
    with pytest.raises(GnmsError):                                       # ranked runs outside 2048 < N <= 4096: an error, no other sort
        _sorts(lib, _scores(rng, 2, 2048), None, None, 2)
    with pytest.raises(GnmsError):
        _sorts(lib, _scores(rng, 2, 4097), None, None, 2)


def test_recycled_workspace(lib):
    """No flag or counter depends on what an earlier launch left: a workspace full of 0xFF bytes, two calls with different inputs and counts,
    the second must equal the same call on a fresh workspace."""
    B, N = 3, 2112
    rng = np.random.default_rng(6)
    s1, b1, c1 = -np.sort(-_scores(rng, B, N), axis=1), _uniform(rng, B, N), np.array([N, 0, 1], np.int32)
    b1[0, 5, 2] = b1[0, 5, 0] - 1.0                                     # (first call: sorted scores, one box that is not plain)
    s2, b2, c2 = _scores(rng, B, N), _uniform(rng, B, N), np.array([N - 1, 256, 257], np.int32)
    for route in (2, 1):
        ws = _workspace(lib, B, N, fill=0xFF)
        first = _sorts(lib, s1, b1, c1, route, ws)
        assert first["flags"][0].tolist() == [1, 1]
        second = _sorts(lib, s2, b2, c2, route, ws)
        _same(second, _sorts(lib, s2, b2, c2, route), ("recycled", route))
        _check_numpy(second, s2, b2, c2, ("recycled", route))


_END_TO_END = """
import sys, numpy as np, torch
import groomed_nms_amd as G
from groomed_nms_amd import synthetic, overlaps
out = {}
def keep(tag, o, st):
    w = torch.linspace(-1.0, 2.0, o[0].shape[1], device="cuda").repeat(o[0].shape[0], 1)
    (o[0] * w).sum().backward()
    for i in range(6):
        out["%s_%d" % (tag, i)] = o[i].detach().cpu().numpy()
    out[tag + "_grad"], out[tag + "_w"] = st.grad.cpu().numpy().copy(), w[0].cpu().numpy()
for tag, B, N, kind in (("one_2112", 3, 2112, "uniform"), ("one_4096", 8, 4096, "clustered")):
    b, s = synthetic.batch_2d(21, B, N, kind)
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    keep(tag, G.differentiable_nms_with_iou2d_batched(st, torch.from_numpy(b).cuda()), st)
b, s = synthetic.batch_2d(21, 3, 2112, "uniform")
st = torch.from_numpy(s).cuda().requires_grad_(True)
keep("two_2112", G.differentiable_nms_batched(st, overlaps.iou_batched(torch.from_numpy(b).cuda())), st)
p3, s3 = synthetic.batch_3d(22, 3, 2112, clustered=True)
st = torch.from_numpy(s3).cuda().requires_grad_(True)
keep("d3_2112", G.differentiable_nms_with_iou3d_batched(st, torch.from_numpy(p3).cuda()), st)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print("ok")
"""


def test_end_to_end_against_runs_and_merge(tmp_path):
    """GNMS_RANK_SORT=0 (runs + merge) against the default, in child processes (the switch is read once): outputs 0-5 and grad_scores of the
    one-call 2D layer, the matrix-in layer and the 3D layer (mode3d bands, xrec) bit for bit; and the default run against the oracle."""
    from groomed_nms_amd import synthetic
    from oracle import oracle as O
    runs = {}
    for tag, env in (("default", {}), ("runs_merge", {"GNMS_RANK_SORT": "0"})):
        path = str(tmp_path / ("sorts_%s.npz" % tag))
        r = subprocess.run([sys.executable, "-c", _END_TO_END, path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, (tag, r.stderr[-2000:])
        runs[tag] = np.load(path)
    assert len(runs["default"].files) == 4 * 8
    for k in runs["default"].files:
        assert runs["default"][k].tobytes() == runs["runs_merge"][k].tobytes(), k
    d = runs["default"]
    b, s = synthetic.batch_2d(21, 3, 2112, "uniform")
    w = d["one_2112_w"]
    for i in range(2):                                                   # tolerance 0
        ref = O.differentiable_nms(s[i], O.iou2d(b[i], b[i]), grad_prob=w)
        assert np.array_equal(d["one_2112_0"][i], ref["prob"]), i
        assert d["one_2112_2"][i, :int(d["one_2112_4"][i])].tolist() == list(ref["valid"]), i
        assert np.array_equal(d["one_2112_grad"][i], ref["grad_scores"]), i
