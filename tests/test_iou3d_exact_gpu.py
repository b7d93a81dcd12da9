"""The exact rotated IoU on the MI355X (csrc/iou3d_exact.hip): gnms_iou3d_exact / _from_params (fp32 matrices) and
gnms_iou3d_exact_list_f64 (the iou3d drop-in) against known answers, against the independent float64 checker of
test_iou3d_exact_host.py, against the pinned oracle where the boxes are axis-aligned, and under graph capture.

Bounds: |fp32 - checker| <= 2e-7 (the output rounding of a value in [0, 1] is <= 3e-8), |f64 - checker| <= 1e-12."""
import math

import numpy as np
import pytest
import torch

from test_iou3d_exact_host import (analytic_cases, checker_matrix, clockwise, corners, exact_iou, touching_pair,
                                   aabb_volume)

pytestmark = pytest.mark.gpu

F32_TOL = 2e-7
F64_TOL = 1e-12


@pytest.fixture(scope="module")
def ov():
    from groomed_nms_amd import _lib, overlaps
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return overlaps


def own_volume(c):
    f = [(c[0, i], c[2, i]) for i in (7, 2, 3, 6)]
    a = abs(0.5 * sum(f[i][0] * f[(i + 1) % 4][1] - f[(i + 1) % 4][0] * f[i][1] for i in range(4)))
    return a * (c[1].max() - c[1].min())


def matrix(ov, ca, cb, volume, want=("bev", "3d"), ld_pad=0, from_params=False):
    """one fp32 call on [B, M, .] x [B, N, .] with the outputs requested by `want`, row stride N + ld_pad -> numpy (bev, i3) or None"""
    from groomed_nms_amd import _lib
    a = torch.from_numpy(np.ascontiguousarray(ca, np.float32)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(cb, np.float32)).cuda()
    B, M, N = a.shape[0], a.shape[1], b.shape[1]
    ld = N + ld_pad
    bev = torch.full((B, M, ld), -7.0, device="cuda") if "bev" in want else None
    i3 = torch.full((B, M, ld), -7.0, device="cuda") if "3d" in want else None
    fn = _lib.load().gnms_iou3d_exact_from_params if from_params else _lib.load().gnms_iou3d_exact
    _lib.check(fn(_lib.ptr(a), _lib.ptr(b), B, M, N, {"box": 0, "aabb": 1}[volume], _lib.ptr(bev), _lib.ptr(i3), ld,
                  _lib.stream_ptr()), "gnms_iou3d_exact")
    torch.cuda.synchronize()
    out = []
    for t in (bev, i3):
        if t is None:
            out.append(None)
            continue
        t = t.cpu().numpy()
        assert (t[:, :, N:] == -7.0).all(), "a write beyond column N"
        out.append(t[:, :, :N].astype(np.float64))
    return out


def assert_close(got, want, tol, what):
    bad = ~((np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d entries off, max |d| = %.3g, first at %s: got %r want %r"
                             % (what, bad.sum(), np.nanmax(np.abs(got - want)), tuple(k), got[tuple(k)], want[tuple(k)]))


# ---------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------
def test_known_answers(ov):
    cases = analytic_cases()
    ca = np.stack([c[1] for c in cases])
    cb = np.stack([c[2] for c in cases])
    vol = np.array([own_volume(a) + own_volume(b) for a, b in zip(ca, cb)])
    want_bev = np.array([c[3] for c in cases])
    want_3d = np.array([c[4] for c in cases])
    names = [c[0] for c in cases]
    # the f64 drop-in, both orientations of either footprint
    for a_, b_ in ((ca, cb), (np.stack([clockwise(a) for a in ca]), cb), (ca, np.stack([clockwise(b) for b in cb]))):
        bev, i3 = ov.iou3d(a_, b_, vol=vol)
        for k, n in enumerate(names):
            assert abs(bev[k] - want_bev[k]) <= F64_TOL and abs(i3[k] - want_3d[k]) <= F64_TOL, (n, bev[k], i3[k])
    # exactly 0 for disjoint and edge-sharing boxes
    for n in ("disjoint", "touching_edge", "touching_edge_rotated"):
        k = names.index(n)
        assert bev[k] == 0.0 and i3[k] == 0.0, (n, bev[k], i3[k])
    # the fp32 matrix on the same boxes rounded to fp32: against the checker on those fp32 corners (the diagonal), and the checker
    # against the analytic value
    a32, b32 = ca.astype(np.float32), cb.astype(np.float32)
    for ccw_a in (False, True):
        aa = np.stack([clockwise(a) for a in a32]) if ccw_a else a32
        bev_m, i3_m = matrix(ov, aa[None], b32[None], "box")
        for k, n in enumerate(names):
            wb, w3 = exact_iou(aa[k].astype(np.float64), b32[k].astype(np.float64), volume="box")
            assert abs(bev_m[0, k, k] - wb) <= F32_TOL and abs(i3_m[0, k, k] - w3) <= F32_TOL, (n, bev_m[0, k, k], wb, i3_m[0, k, k], w3)
            assert abs(wb - want_bev[k]) <= 2e-6 and abs(w3 - want_3d[k]) <= 2e-6, (n, wb, w3)
        for n in ("disjoint", "touching_edge", "touching_edge_rotated"):
            k = names.index(n)
            assert bev_m[0, k, k] == 0.0 and i3_m[0, k, k] == 0.0, n
        for n in ("identical", "identical_rotated"):
            k = names.index(n)
            assert abs(bev_m[0, k, k] - 1.0) <= F32_TOL, (n, bev_m[0, k, k])


def test_special_values(ov):
    z = corners(1, 1, 1, 0.0, 1, 0.0, 0.3)                          # zero footprint area
    bev, i3 = ov.iou3d(z, z)
    assert math.isnan(bev) and math.isnan(i3)
    bev_m, i3_m = matrix(ov, z[None, None], z[None, None], "box")
    assert np.isnan(bev_m).all() and np.isnan(i3_m).all()
    # vol=None, a rotated box against itself: the reference's AABB volumes
    c = corners(2, 1, 8, 1.6, 1.5, 3.9, 0.6)
    bev, i3 = ov.iou3d(c, c)
    a, h = 1.6 * 3.9, 1.5
    assert abs(bev - 1.0) <= F64_TOL and abs(i3 - a * h / (2 * aabb_volume(c) - a * h)) <= F64_TOL, (bev, i3)
    assert isinstance(bev, np.float64) and isinstance(i3, np.float64)
    bev_m, i3_m = matrix(ov, c[None, None], c[None, None], "aabb")
    assert abs(bev_m[0, 0, 0] - 1.0) <= F32_TOL and abs(i3_m[0, 0, 0] - a * h / (2 * aabb_volume(c) - a * h)) <= F32_TOL
    # disjoint y ranges: iou_3d = 0, iou_bev as in BEV
    c2 = corners(2, 5, 8, 1.6, 1.5, 3.9, 0.6)
    bev, i3 = ov.iou3d(c, c2)
    assert abs(bev - 1.0) <= F64_TOL and i3 == 0.0
    bev_m, i3_m = matrix(ov, c[None, None], c2[None, None], "box")
    assert abs(bev_m[0, 0, 0] - 1.0) <= F32_TOL and i3_m[0, 0, 0] == 0.0
    _, i3_only = matrix(ov, c[None, None], c2[None, None], "box", want=("3d",))
    assert i3_only[0, 0, 0] == 0.0
    # inputs are not modified, scalar vol broadcast over a batch
    cc = np.stack([c, c2])
    keep = cc.copy()
    bev, i3 = ov.iou3d(cc, cc[::-1].copy(), vol=10.0)
    assert np.array_equal(cc, keep) and bev.shape == (2,) and i3.shape == (2,)


# ---------------------------------------------------------------------------------------------------------------------------
# random parity against the checker
# ---------------------------------------------------------------------------------------------------------------------------
def corner_sets(ov, seed, B, M, N, clustered):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    pa = np.stack([synthetic.boxes_3d(rng, M, clustered, per=16) for _ in range(B)])
    pb = np.stack([synthetic.boxes_3d(rng, N, clustered, per=16) for _ in range(B)])
    ca = ov.corners_batched(torch.from_numpy(pa).cuda()).cpu().numpy()
    cb = ov.corners_batched(torch.from_numpy(pb).cuda()).cpu().numpy()
    return pa, pb, ca, cb


SHAPES = [(1, 1, 1), (1, 7, 300), (3, 64, 257), (1, 263, 1100), (3, 500, 33), (1, 9, 511), (3, 130, 200)]


@pytest.mark.parametrize("clustered", [False, True], ids=["uniform", "clustered"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dM%dN%d" % s)
def test_random_parity(ov, shape, clustered):
    B, M, N = shape
    seed = 1000 * B + 7 * M + N + int(clustered)
    pa, pb, ca, cb = corner_sets(ov, seed, B, M, N, clustered)
    want = {v: [checker_matrix(ca[b], cb[b], volume=v) for b in range(B)] for v in ("box", "aabb")}
    for k, (volume, outs, pad) in enumerate((("box", ("bev", "3d"), 0), ("aabb", ("bev", "3d"), 5), ("box", ("bev",), 3),
                                             ("aabb", ("3d",), 0), ("box", ("3d",), 1))):
        bev, i3 = matrix(ov, ca, cb, volume, want=outs, ld_pad=pad)
        for b in range(B):
            wb, w3 = want[volume][b]
            tag = "seed %d B%d M%d N%d volume %s outputs %s ld N+%d image %d" % (seed, B, M, N, volume, outs, pad, b)
            if bev is not None:
                assert_close(bev[b], wb, F32_TOL, "iou_bev " + tag)
            if i3 is not None:
                assert_close(i3[b], w3, F32_TOL, "iou_3d " + tag)
    # from params == corners then exact, bit for bit
    for volume in ("box", "aabb"):
        m1 = matrix(ov, pa, pb, volume, from_params=True)
        m2 = matrix(ov, ca, cb, volume)
        for x, y in zip(m1, m2):
            assert np.array_equal(x, y, equal_nan=True), "from_params differs from corners, seed %d volume %s" % (seed, volume)
    # the f64 drop-in on the diagonal pairs (the same fp32 corners widened), and the fp32 diagonal against it
    n = min(M, N)
    for b in range(B):
        bev, i3 = ov.iou3d(ca[b, :n].astype(np.float64), cb[b, :n].astype(np.float64))
        wb, w3 = want["aabb"][b]
        assert_close(bev, np.diagonal(wb[:n, :n]), F64_TOL, "f64 iou_bev seed %d image %d" % (seed, b))
        assert_close(i3, np.diagonal(w3[:n, :n]), F64_TOL, "f64 iou_3d seed %d image %d" % (seed, b))
        mb, m3 = matrix(ov, ca[b:b + 1, :n], cb[b:b + 1, :n], "aabb")
        assert_close(np.diagonal(mb[0]), bev, F32_TOL, "drop-in vs combinations diagonal (bev) seed %d" % seed)
        assert_close(np.diagonal(m3[0]), i3, F32_TOL, "drop-in vs combinations diagonal (3d) seed %d" % seed)


@pytest.mark.parametrize("seed", [11, 12])
def test_near_identical_perturbations(ov, seed):
    """identical boxes nudged by tiny rotations, shifts and size changes: near-parallel and near-touching edges"""
    rng = np.random.default_rng(seed)
    from groomed_nms_amd import synthetic
    base = synthetic.boxes_3d(rng, 64).astype(np.float64)
    rows_a, rows_b = [], []
    for p in base:
        for kind in range(6):
            q = p.copy()
            e = 10.0 ** rng.uniform(-9, -3)
            if kind == 0:
                q[6] += e                                               # near-parallel edges
            elif kind == 1:
                q[0] += e * math.cos(p[6]); q[2] -= e * math.sin(p[6])  # near-collinear long edges
            elif kind == 2:
                q[3] *= 1 + e                                           # near-coincident sides
            elif kind == 3:                                             # near-touching along the width: shifted by w (+- e)
                s = p[3] + e * rng.choice([-1, 1])
                q[0] += s * math.sin(p[6]); q[2] += s * math.cos(p[6])
            elif kind == 4:                                             # near-touching along the length
                s = p[5] + e * rng.choice([-1, 1])
                q[0] += s * math.cos(p[6]); q[2] -= s * math.sin(p[6])
            rows_a.append(p)
            rows_b.append(q)
    ca = np.stack([corners(*r) for r in rows_a])
    cb = np.stack([corners(*r) for r in rows_b])
    for volume in ("box", "aabb"):
        vol = None if volume == "aabb" else np.array([own_volume(a) + own_volume(b) for a, b in zip(ca, cb)])
        bev, i3 = ov.iou3d(ca, cb, vol=vol)
        want = np.array([exact_iou(a, b, volume=volume) for a, b in zip(ca, cb)])
        assert_close(bev, want[:, 0], F64_TOL, "f64 iou_bev, seed %d volume %s" % (seed, volume))
        assert_close(i3, want[:, 1], F64_TOL, "f64 iou_3d, seed %d volume %s" % (seed, volume))
        # fp32 corners in one matrix call (every pair of the set, the checker on the fp32 corners)
        a32, b32 = ca.astype(np.float32), cb.astype(np.float32)
        mb, m3 = matrix(ov, a32[None], b32[None], volume)
        wb, w3 = checker_matrix(a32.astype(np.float64), b32.astype(np.float64), volume=volume)
        assert_close(mb[0], wb, F32_TOL, "fp32 iou_bev, seed %d volume %s" % (seed, volume))
        assert_close(m3[0], w3, F32_TOL, "fp32 iou_3d, seed %d volume %s" % (seed, volume))


# ---------------------------------------------------------------------------------------------------------------------------
# cross-checks, scale, capture
# ---------------------------------------------------------------------------------------------------------------------------
def test_axis_aligned_matches_oracle_approximate(ov):
    """ry = 0 everywhere: the exact and the approximate IoU coincide; volume_mode 1 (AABB volumes) against the pinned oracle"""
    from oracle import oracle as O
    seed = 21
    for clustered in (False, True):
        pa, pb, _, _ = corner_sets(ov, seed, 1, 300, 410, clustered)
        pa[..., 6] = 0.0
        pb[..., 6] = 0.0
        ca = ov.corners_batched(torch.from_numpy(pa).cuda()).cpu().numpy()
        cb = ov.corners_batched(torch.from_numpy(pb).cuda()).cpu().numpy()
        bev, i3 = matrix(ov, ca, cb, "aabb")
        ob, o3 = O.iou3d_approximate(ca[0], cb[0], generalized=False)
        assert_close(bev[0], ob.astype(np.float64), 1e-6, "iou_bev vs oracle, seed %d clustered %s" % (seed, clustered))
        assert_close(i3[0], o3.astype(np.float64), 1e-6, "iou_3d vs oracle, seed %d clustered %s" % (seed, clustered))
        assert (bev[0] > 0).sum() > 50


def test_scale_b8_n4096_sampled(ov):
    seed = 31
    B, N = 8, 4096
    pa, _, ca, _ = corner_sets(ov, seed, B, N, 1, True)
    a = torch.from_numpy(pa).cuda()
    bev_t, i3_t = ov.iou3d_exact_batched(a, from_params=True, want_bev=True)
    torch.cuda.synchronize()
    bev, i3 = bev_t.cpu().numpy().astype(np.float64), i3_t.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(seed)
    bi, ri, cj = rng.integers(0, B, 20000), rng.integers(0, N, 20000), rng.integers(0, N, 20000)
    got_b, got_3 = bev[bi, ri, cj], i3[bi, ri, cj]
    want = np.array([exact_iou(ca[b, r], ca[b, c], volume="box") for b, r, c in zip(bi, ri, cj)])
    assert_close(got_b, want[:, 0], F32_TOL, "sampled iou_bev, seed %d" % seed)
    assert_close(got_3, want[:, 1], F32_TOL, "sampled iou_3d, seed %d" % seed)
    for b, r in zip(rng.integers(0, B, 64), rng.integers(0, N, 64)):
        wb, w3 = checker_matrix(ca[b, r:r + 1], ca[b], volume="box")
        assert_close(bev[b, r:r + 1], wb, F32_TOL, "row %d of image %d, seed %d (bev)" % (r, b, seed))
        assert_close(i3[b, r:r + 1], w3, F32_TOL, "row %d of image %d, seed %d (3d)" % (r, b, seed))
    assert np.all(np.abs(np.diagonal(bev, axis1=1, axis2=2) - 1.0) <= F32_TOL)


def test_graph_capture_equals_eager(ov):
    _, _, ca, cb = corner_sets(ov, 41, 2, 700, 900, True)
    a = torch.from_numpy(ca).cuda()
    b = torch.from_numpy(cb).cuda()
    eager = ov.iou3d_exact_batched(a, b, volume="aabb", want_bev=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ov.iou3d_exact_batched(a, b, volume="aabb", want_bev=True)        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ov.iou3d_exact_batched(a, b, volume="aabb", want_bev=True)
    for t in captured:
        t.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(captured, eager):
        assert torch.equal(torch.nan_to_num(x, nan=-5.0), torch.nan_to_num(y, nan=-5.0))
