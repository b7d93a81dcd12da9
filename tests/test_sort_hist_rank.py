"""The histogram sort of 2048 < N <= 4096 keys per image (sort_hist_rank_kernel: bin by a monotone function of the key, scan, scatter into bin
order, count the smaller keys of the key's own bin) against the two-launch runs + merge.  Everything on the GPU goes through
gnms_profile_sorts in one process: route 3 against route 1 bit for bit on every array the sorts leave behind and on both flags, and on plain
inputs against NumPy's stable sorts.  The keys are distinct (the index is in the low bits), so the order is unique and there is nothing to
tolerate.  gnms_profile_sort_paths says which way each image and role went (by histogram, or the run-sort fallback past `cap` keys in a bin).
The bin function itself (csrc/sort_bins.h) is checked on the host, without a GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARRAYS = ("order", "rankof", "sscore", "rbox", "xidx", "xbox", "flags")
# (B, N): one real key in the ninth 256 and nothing behind; 2112; one key short of full; full; 288 workgroups with boxes (more than one round)
SHAPES = ((3, 2049), (3, 2112), (3, 4095), (3, 4096), (9, 2304))
BY_HIST, FELL_BACK = 1, 2


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


def _paths(lib, ws, B, N):
    """([B][2] paths of the last histogram sort on `ws`, the cap)"""
    from groomed_nms_amd._lib import check, ptr, stream_ptr
    p = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    cap = ctypes.c_int32(-1)
    check(lib.gnms_profile_sort_paths(B, N, ptr(p), ctypes.byref(cap), ptr(ws), ws.numel(), stream_ptr()), "gnms_profile_sort_paths")
    torch.cuda.synchronize()
    return p.cpu().numpy(), int(cap.value)


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
    res = {k: v.cpu().numpy() for k, v in o.items()}
    if route == 3:
        res["paths"], res["cap"] = _paths(lib, ws, B, N)
    return res


def _same(a, b, what):
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _both(lib, scores, boxes, counts, what):
    """Route 3 against route 1, bit for bit; returns the histogram sort's result (with its paths)."""
    one = _sorts(lib, scores, boxes, counts, 1)
    three = _sorts(lib, scores, boxes, counts, 3)
    _same(three, one, what)
    assert np.isin(three["paths"][:, :2 if boxes is not None else 1], (BY_HIST, FELL_BACK)).all(), (what, three["paths"])
    return three


def _plain(b):
    """box_orders_plainly: finite coordinates, no negative zero, x2 >= x1, y2 >= y1"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(b).all(-1) & ~((b == 0) & np.signbit(b)).any(-1) & (b[..., 2] >= b[..., 0]) & (b[..., 3] >= b[..., 1])


def _check_numpy(res, scores, boxes, counts, what, check_order=True, check_x=True):
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
        if check_x:
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


def _most_equal(values, counts):
    """per image: the largest number of equal values among its first n (they share a bin whatever the bins are)"""
    B, N = values.shape
    return np.array([max(np.unique(values[b, :n], return_counts=True)[1], default=0) for b, n in enumerate(_ns(counts, B, N))])


@gpu
@pytest.mark.parametrize("with_boxes", (True, False), ids=("boxes", "scores_alone"))
@pytest.mark.parametrize("B,N", SHAPES)
def test_scores(lib, B, N, with_boxes):
    rng = np.random.default_rng(1300 + N)
    boxes = _uniform(rng, B, N) if with_boxes else None
    rnd = _scores(rng, B, N)
    desc = -np.sort(-rnd, axis=1)
    skew = (1.0 / (1.0 + np.exp(-rng.normal(-4.0, 2.0, size=(B, N))))).astype(np.float32)   # a detector's scores: most of them near zero
    for counts in _counts(B, N):
        ns = np.array(_ns(counts, B, N))
        tag = (B, N, None if counts is None else counts[:3].tolist())
        res = _both(lib, rnd, boxes, counts, tag + ("random",))
        _check_numpy(res, rnd, boxes, counts, tag + ("random",))
        cap = res["cap"]
        assert 16 <= cap <= 4096, cap
        assert (res["paths"][:, :2 if with_boxes else 1] == BY_HIST).all(), tag + ("uniform inputs go by histogram", res["paths"])
        res = _both(lib, desc, boxes, counts, tag + ("descending",))
        _check_numpy(res, desc, boxes, counts, tag + ("descending",))
        assert (res["flags"][:, 0] == 1).all(), tag
        for where in ("front", "edge of 256", "back"):                   # descending except for one swap
            sw = desc.copy()
            hit = []
            for b, n in enumerate(ns):
                i = {"front": 0, "edge of 256": 255, "back": n - 2}[where]
                if 0 <= i and i + 1 < n:
                    sw[b, [i, i + 1]] = sw[b, [i + 1, i]]
                    hit.append(b)
            res = _both(lib, sw, boxes, counts, tag + (where,))
            _check_numpy(res, sw, boxes, counts, tag + (where,))
            assert (res["flags"][np.array(hit, dtype=int), 0] == 0).all(), tag + (where,)
        _check_numpy(_both(lib, skew, boxes, counts, tag + ("skewed",)), skew, boxes, counts, tag + ("skewed",))
        equal = np.full((B, N), 0.5, np.float32)                         # lo == hi: one bin
        res = _both(lib, equal, boxes, counts, tag + ("equal",))
        _check_numpy(res, equal, boxes, counts, tag + ("equal",))
        assert np.array_equal(res["order"], np.tile(np.arange(N, dtype=np.int32), (B, 1))) and (res["flags"][:, 0] == 1).all(), tag
        assert np.array_equal(res["paths"][:, 0] == FELL_BACK, ns > cap), tag + ("equal", res["paths"])
        three = (rng.integers(0, 3, size=(B, N)) / 4.0).astype(np.float32)   # three values: stable among ties, and the fallback
        res = _both(lib, three, boxes, counts, tag + ("three values",))
        _check_numpy(res, three, boxes, counts, tag + ("three values",))
        big = _most_equal(three, counts) > cap                           # (the three values lie bins apart: a bin holds what is equal)
        assert np.array_equal(res["paths"][:, 0] == FELL_BACK, big) and big[ns >= 2049].all(), tag + ("three values", res["paths"])
        # exactly cap and cap + 1 equal scores (2.0, a bin to themselves: everything else is below 1, half the range away) among distinct ones
        for extra in (0, 1):
            ce = rnd.copy()
            full = []
            for b, n in enumerate(ns):
                if n > 4 * cap:
                    ce[b, rng.choice(n, cap + extra, replace=False)] = 2.0
                    full.append(b)
            res = _both(lib, ce, boxes, counts, tag + ("cap + %d" % extra,))
            _check_numpy(res, ce, boxes, counts, tag + ("cap + %d" % extra,))
            assert (res["paths"][np.array(full, dtype=int), 0] == (FELL_BACK if extra else BY_HIST)).all(), tag + ("cap + %d" % extra, res["paths"])
        special = rnd.copy()                                             # against runs + merge only
        pick = rng.integers(0, 6, size=(B, N))
        for v, val in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):
            special[pick == v] = val
        res = _both(lib, special, boxes, counts, tag + ("special",))
        _check_numpy(res, special, boxes, counts, tag + ("special",), check_order=False)
        few = rnd.copy()                                                 # one of each, below the cap: these go by histogram
        for b, n in enumerate(ns):
            if n >= 64:
                few[b, rng.choice(n, 5, replace=False)] = (np.nan, np.inf, -np.inf, 0.0, -0.0)
        res = _both(lib, few, boxes, counts, tag + ("few specials",))
        _check_numpy(res, few, boxes, counts, tag + ("few specials",), check_order=False)
        assert (res["paths"][:, 0] == BY_HIST).all(), tag + ("few specials", res["paths"])


@gpu
@pytest.mark.parametrize("B,N", SHAPES)
def test_boxes(lib, B, N):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(2300 + N)
    scores = _scores(rng, B, N)
    uniform = _uniform(rng, B, N)
    clustered = np.stack([synthetic.clustered_boxes_2d(rng, N, 32) for _ in range(B)]).astype(np.float32)   # (x centres below zero among them)
    blocks = uniform.copy()                                              # equal x centres in blocks of 300: ties go by index
    cx = np.repeat(rng.permutation((N + 299) // 300), 300)[:N].astype(np.float32) * 8.0
    blocks[:, :, 0], blocks[:, :, 2] = cx - 4.0, cx + 4.0
    nanx = uniform.copy()                                                # NaN x: these sort last
    nanx[:, rng.choice(N, 40, replace=False), 0] = np.nan
    far = uniform.copy()                                                 # one box at 1e30: every other box in one bin
    far[:, 3, 0], far[:, 3, 2] = 1e30, 1.5e30
    infx = uniform.copy()                                                # x centres of +inf and -inf (not plain)
    infx[:, 9, 2], infx[:, 11, 0] = np.inf, -np.inf
    for counts in _counts(B, N):
        ns = np.array(_ns(counts, B, N))
        tag = (B, N, None if counts is None else counts[:3].tolist())
        for name, bx in (("uniform", uniform), ("clustered", clustered), ("blocks", blocks), ("nan x", nanx), ("far", far), ("inf x", infx)):
            res = _both(lib, scores, bx, counts, tag + (name,))
            _check_numpy(res, scores, bx, counts, tag + (name,), check_x=name != "inf x")   # (NumPy's inf - inf centres: against runs + merge only)
            cap = res["cap"]
            if name in ("uniform", "clustered", "blocks", "far"):
                assert (res["flags"][:, 1] == 0).all(), tag + (name,)     # no box that is not plain
            assert (res["paths"][:, 0] == BY_HIST).all(), tag + (name, res["paths"])
            if name == "uniform":
                assert (res["paths"][:, 1] == BY_HIST).all(), tag + (name, res["paths"])
            if name == "blocks":                                         # up to 300 equal centres, the blocks bins apart
                assert np.array_equal(res["paths"][:, 1] == FELL_BACK, _most_equal(bx[:, :, 0] + bx[:, :, 2], counts) > cap), tag + (name, res["paths"])
            if name == "far":                                            # with box 3 among them, every other box is in the first bin
                assert np.array_equal(res["paths"][:, 1] == FELL_BACK, ns - (ns > 3) > cap), tag + (name, res["paths"])
        for kind in ("x2 < x1", "nan", "minus zero"):                    # ONE box that is not plain, per image
            for where in ("first 256", "last 256", "last"):
                bx = uniform.copy()
                hit = []
                for b, n in enumerate(ns):
                    i = {"first 256": 7, "last 256": 15 * 256 + 7, "last": n - 1}[where]
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


@gpu
def test_routes(lib):
    """Route 0 leaves the same arrays as runs + merge wherever it goes, and route 3 outside 2048 < N <= 4096 is an error, no other sort."""
    rng = np.random.default_rng(135)
    for B, N in ((1, 4096), (3, 2112), (8, 4096), (16, 4096)):
        scores, boxes = _scores(rng, B, N), _uniform(rng, B, N)
        _same(_sorts(lib, scores, boxes, None, 0), _sorts(lib, scores, boxes, None, 1), (B, N))
        _same(_sorts(lib, scores, None, None, 0), _sorts(lib, scores, None, None, 1), (B, N, "scores alone"))
    from groomed_nms_amd._lib import GnmsError
    with pytest.raises(GnmsError):
        _sorts(lib, _scores(rng, 2, 2048), None, None, 3)
    with pytest.raises(GnmsError):
        _sorts(lib, _scores(rng, 2, 4097), None, None, 3)
    with pytest.raises(GnmsError):                                       # route 2 keeps its range and its error
        _sorts(lib, _scores(rng, 2, 2048), None, None, 2)


@gpu
def test_recycled_workspace(lib):
    """No flag, counter or bin depends on what an earlier launch left: a workspace full of 0xFF bytes, two calls with different inputs and
    counts, the second must equal the same call on a fresh workspace -- by histogram, and through the fallback."""
    B, N = 3, 2112
    rng = np.random.default_rng(136)
    s1, b1, c1 = -np.sort(-_scores(rng, B, N), axis=1), _uniform(rng, B, N), np.array([N, 0, 1], np.int32)
    b1[0, 5, 2] = b1[0, 5, 0] - 1.0                                     # (first call: sorted scores, one box that is not plain)
    s2, b2, c2 = _scores(rng, B, N), _uniform(rng, B, N), np.array([N - 1, 256, 257], np.int32)
    s3 = (rng.integers(0, 3, size=(B, N)) / 4.0).astype(np.float32)
    ws = _workspace(lib, B, N, fill=0xFF)
    first = _sorts(lib, s1, b1, c1, 3, ws)
    assert first["flags"][0].tolist() == [1, 1]
    second = _sorts(lib, s2, b2, c2, 3, ws)
    _same(second, _sorts(lib, s2, b2, c2, 1), "recycled")
    _check_numpy(second, s2, b2, c2, "recycled")
    assert (second["paths"] == BY_HIST).all()
    third = _sorts(lib, s3, b2, c2, 3, ws)                               # ... and the fallback on the same workspace
    _same(third, _sorts(lib, s3, b2, c2, 1), "recycled, fallback")
    assert np.array_equal(third["paths"][:, 0] == FELL_BACK, _most_equal(s3, c2) > third["cap"]) and (third["paths"][:, 0] == FELL_BACK).any()
    assert (third["paths"][:, 1] == BY_HIST).all()
    again = _sorts(lib, s2, b2, c2, 3, ws)
    _same(again, second, "recycled, after the fallback")


@gpu
def test_graph_capture(lib):
    """One capture of the histogram sort, three replays on changed inputs (the third through the fallback)."""
    from groomed_nms_amd._lib import check, ptr, stream_ptr
    B, N = 3, 2112
    rng = np.random.default_rng(137)
    dev = torch.device("cuda")
    ws = _workspace(lib, B, N)
    st, bt = torch.zeros((B, N), device=dev), torch.zeros((B, N, 4), device=dev)
    ct = torch.full((B,), N, dtype=torch.int32, device=dev)
    o = dict(order=torch.zeros((B, N), dtype=torch.int32, device=dev), rankof=torch.zeros((B, N), dtype=torch.int32, device=dev),
             sscore=torch.zeros((B, N), device=dev), rbox=torch.zeros((B, N, 4), device=dev), xidx=torch.zeros((B, N), dtype=torch.int32, device=dev),
             xbox=torch.zeros((B, N, 4), device=dev), flags=torch.zeros((B, 2), dtype=torch.int32, device=dev))

    def call():
        check(lib.gnms_profile_sorts(ptr(st), ptr(bt), B, N, ptr(ct), 3, ptr(o["order"]), ptr(o["rankof"]), ptr(o["sscore"]), ptr(o["rbox"]),
                                     ptr(o["xidx"]), ptr(o["xbox"]), ptr(o["flags"]), ptr(ws), ws.numel(), stream_ptr()), "gnms_profile_sorts")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                           # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for rep in range(3):
        s = _scores(rng, B, N) if rep < 2 else (rng.integers(0, 3, size=(B, N)) / 4.0).astype(np.float32)
        b = _uniform(rng, B, N)
        c = np.array(([N, N, N], [N - 1, 256, 257], [N, 0, 1])[rep], np.int32)
        st.copy_(torch.from_numpy(s)); bt.copy_(torch.from_numpy(b)); ct.copy_(torch.from_numpy(c))
        for v in o.values():
            v.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        _same(got, _sorts(lib, s, b, c, 1), ("replay", rep))
        paths, _ = _paths(lib, ws, B, N)
        assert paths[0, 0] == (FELL_BACK if rep == 2 else BY_HIST), (rep, paths)
    del g


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
for tag, B, N, kind in (("one_2112", 3, 2112, "uniform"), ("one_4096", 8, 4096, "uniform"), ("one_4096c", 8, 4096, "clustered")):
    b, s = synthetic.batch_2d(131, B, N, kind)
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    keep(tag, G.differentiable_nms_with_iou2d_batched(st, torch.from_numpy(b).cuda()), st)
for tag, B in (("two_2112", 3), ("two_2112_b16", 16)):                  # (3 images: by counting; 16: the one-launch sort of the scores alone)
    b, s = synthetic.batch_2d(131, B, 2112, "uniform")
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    keep(tag, G.differentiable_nms_batched(st, overlaps.iou_batched(torch.from_numpy(b).cuda())), st)
for tag, B in (("d3_2112", 2), ("d3_2112_b8", 8)):                      # (2 images: by counting; 8: the one-launch sort with four z bands)
    p3, s3 = synthetic.batch_3d(132, B, 2112, clustered=True)
    st = torch.from_numpy(s3).cuda().requires_grad_(True)
    keep(tag, G.differentiable_nms_with_iou3d_batched(st, torch.from_numpy(p3).cuda()), st)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print("ok")
"""


@gpu
def test_end_to_end_against_switch_off(tmp_path):
    """The default against GNMS_HIST_SORT=0 in child processes (the switch is read once): outputs 0-5 and grad_scores of the one-call 2D layer,
    the matrix-in layer and the 3D layer (z bands, xrec) bit for bit; and the default run against the oracle at tolerance 0."""
    from groomed_nms_amd import synthetic
    from oracle import oracle as O
    runs = {}
    for tag, env in (("default", {}), ("switch_off", {"GNMS_HIST_SORT": "0"})):
        path = str(tmp_path / ("sorts_%s.npz" % tag))
        r = subprocess.run([sys.executable, "-c", _END_TO_END, path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, (tag, r.stderr[-2000:])
        runs[tag] = np.load(path)
    assert len(runs["default"].files) == 7 * 8
    for k in runs["default"].files:
        assert runs["default"][k].tobytes() == runs["switch_off"][k].tobytes(), k
    d = runs["default"]
    for tag, B, N, imgs in (("one_2112", 3, 2112, (0, 1)), ("one_4096", 8, 4096, (7,))):
        b, s = synthetic.batch_2d(131, B, N, "uniform")
        w = d[tag + "_w"]
        for i in imgs:                                                   # tolerance 0
            ref = O.differentiable_nms(s[i], O.iou2d(b[i], b[i]), grad_prob=w)
            assert np.array_equal(d[tag + "_0"][i], ref["prob"]), (tag, i)
            assert d[tag + "_2"][i, :int(d[tag + "_4"][i])].tolist() == list(ref["valid"]), (tag, i)
            assert np.array_equal(d[tag + "_grad"][i], ref["grad_scores"]), (tag, i)


_HOST_CHECK = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "sort_bins.h"

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static float from_bits(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }
// the sort's keys (gnms_desc_key; column_key's x part is its complement): scores descending with NaN first, x centres ascending with NaN last
static uint32_t desc_key(float v) {
    if (v != v) return 0u;
    const uint32_t u = bits(v + 0.0f);
    const uint32_t asc = (u >> 31) ? ~u : (u | 0x80000000u);
    return ~asc;
}
static int fails = 0;
static void walk(const char* what, std::vector<float> vals, unsigned nb) {
    float lo = std::numeric_limits<float>::infinity(), hi = -lo;
    for (float v : vals) if (std::fabs(v) < std::numeric_limits<float>::infinity()) { lo = std::min(lo, v); hi = std::max(hi, v); }
    const float scale = hist_bin_scale(lo, hi, nb);
    for (int role = 0; role < 2; ++role) {
        std::vector<std::pair<uint32_t, float>> keyed;
        for (float v : vals) keyed.push_back({role == 0 ? desc_key(v) : ~desc_key(v), v});
        std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<uint32_t, float>& a, const std::pair<uint32_t, float>& b) { return a.first < b.first; });
        unsigned prev = 0u;
        for (size_t i = 0; i < keyed.size(); ++i) {
            const float v = keyed[i].second;
            const unsigned bin = role == 0 ? hist_bin_desc(v, lo, scale, nb) : hist_bin_asc(v, lo, scale, nb);
            if (bin >= nb || bin < prev) {
                if (fails++ < 10) std::printf("FAIL %s role %d nb %u at %zu: value %.9g (%08x) bin %u after bin %u, lo %.9g scale %.9g\n", what, role, nb, i, v, bits(v), bin, prev, lo, scale);
            }
            prev = bin;
        }
        // equal keys share a bin (either zero; every NaN)
        for (size_t i = 1; i < keyed.size(); ++i)
            if (keyed[i].first == keyed[i - 1].first) {
                const unsigned a = role == 0 ? hist_bin_desc(keyed[i].second, lo, scale, nb) : hist_bin_asc(keyed[i].second, lo, scale, nb);
                const unsigned c = role == 0 ? hist_bin_desc(keyed[i - 1].second, lo, scale, nb) : hist_bin_asc(keyed[i - 1].second, lo, scale, nb);
                if (a != c && fails++ < 10) std::printf("FAIL %s role %d: equal keys in bins %u and %u\n", what, role, a, c);
            }
    }
}
int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const std::vector<float> special = {nan, inf, -inf, 0.0f, -0.0f, from_bits(0xffc00001u), from_bits(1u), from_bits(0x80000001u), from_bits(0x007fffffu)};
    std::mt19937 gen(13);
    for (unsigned nb : {512u, 2048u, 4096u, 8192u}) {
        for (int set = 0; set < 9; ++set) {
            std::vector<float> v;
            std::uniform_real_distribution<float> u01(0.0f, 1.0f), sym(-900.0f, 2700.0f);
            std::normal_distribution<float> nrm(-4.0f, 2.0f);
            const char* what = "";
            switch (set) {
                case 0: what = "uniform"; for (int i = 0; i < 4096; ++i) v.push_back(u01(gen)); break;
                case 1: what = "across zero"; for (int i = 0; i < 4096; ++i) v.push_back(sym(gen)); break;
                case 2: what = "sigmoid"; for (int i = 0; i < 4096; ++i) v.push_back(1.0f / (1.0f + std::exp(-nrm(gen)))); break;
                case 3: what = "denormals"; for (int i = 0; i < 4096; ++i) v.push_back(from_bits((gen() & 0x807fffffu))); break;
                case 4: what = "lo == hi"; for (int i = 0; i < 100; ++i) v.push_back(0.5f); break;
                case 5: what = "range 1e30"; for (int i = 0; i < 4096; ++i) v.push_back(sym(gen)); v.push_back(1e30f); v.push_back(-1e30f); break;
                case 6: what = "range past FLT_MAX"; for (int i = 0; i < 4096; ++i) v.push_back(sym(gen)); v.push_back(3e38f); v.push_back(-3e38f); break;
                case 7: what = "any bits"; for (int i = 0; i < 4096; ++i) v.push_back(from_bits(gen())); break;
                default: what = "nothing finite"; break;
            }
            walk(what, v, nb);                                           // as drawn ...
            v.insert(v.end(), special.begin(), special.end());
            walk(what, v, nb);                                           // ... and with NaN, +-inf, +-0 and denormals among them
        }
        // a million neighbouring floats around a bin edge: values 0 .. 1, the edge between bins nb / 3 and nb / 3 + 1
        std::vector<float> v = {0.0f, 1.0f};
        float x = (float)(nb / 3 + 1) / (float)nb;
        for (int i = 0; i < 500000; ++i) x = std::nextafter(x, 0.0f);
        for (int i = 0; i < 1000000; ++i) { v.push_back(x); x = std::nextafter(x, 2.0f); }
        std::shuffle(v.begin(), v.end(), gen);
        walk("bin edge", v, nb);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
"""


def test_bin_function_on_the_host(tmp_path):
    """csrc/sort_bins.h compiled alone for the host: for both roles the bins never decrease along sorted keys and stay below the bin count."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "bins.cpp", tmp_path / "bins"
    src.write_text(_HOST_CHECK)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "groomed_nms_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-1000:])
