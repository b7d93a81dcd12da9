"""The exact rotated IoU (lib/core.py:246-302, iou3d) without a GPU: the three C symbols are declared, bound and exported, their
argument checks fail before any HIP call, and the independent float64 checker the GPU tests compare against reproduces the
analytic cases.

The checker is NOT the kernel's algorithm: the intersection polygon is the convex hull (monotone chain) of the vertices of each
footprint that lie inside the other plus every edge-edge intersection point, and its area is the shoelace sum.  Pure NumPy."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gnms_iou3d_exact", "gnms_iou3d_exact_from_params", "gnms_iou3d_exact_list_f64")


# ---------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------
def corners(x, y, z, w, h, l, ry):
    """(3, 8) float64 corners in the reference's iou_3d convention (lib/math_3d.py:364-490)."""
    k = np.arange(8)
    bx = np.where(np.isin(k, (1, 3, 5, 6)), l, 0.0) - l / 2
    by = np.where(np.isin(k, (2, 3, 6, 7)), h, 0.0) - h / 2
    bz = np.where(k >= 4, w, 0.0) - w / 2
    c, s = math.cos(ry), math.sin(ry)
    return np.stack([c * bx + s * bz + x, by + y, -s * bx + c * bz + z])


def clockwise(c):
    """the same box with its footprint 7, 2, 3, 6 traversed the other way (corners 2 and 6 swapped: 7, 6, 3, 2)"""
    c = np.array(c, copy=True)
    c[:, [2, 6]] = c[:, [6, 2]]
    return c


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _hull(points):
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _area(poly):
    n = len(poly)
    return 0.5 * sum(poly[i][0] * poly[(i + 1) % n][1] - poly[(i + 1) % n][0] * poly[i][1] for i in range(n))


def _ccw(quad):
    return quad if _area(quad) >= 0 else quad[::-1]


def _inside(p, quad):
    # on the boundary counts as inside; 1e-12 (m^2, cross-product units) absorbs the rounding of a vertex that lies on an edge line of
    # the other footprint (shared or nearly collinear edges), at an area cost below 1e-12
    return all(_cross(quad[i], quad[(i + 1) % 4], p) >= -1e-12 for i in range(4))


def _segment_hits(p, q, a, b):
    d = (q[0] - p[0]) * (b[1] - a[1]) - (q[1] - p[1]) * (b[0] - a[0])
    if d == 0:
        return []
    t = ((a[0] - p[0]) * (b[1] - a[1]) - (a[1] - p[1]) * (b[0] - a[0])) / d
    u = ((a[0] - p[0]) * (q[1] - p[1]) - (a[1] - p[1]) * (q[0] - p[0])) / d
    if 0 <= t <= 1 and 0 <= u <= 1:
        return [(p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))]
    return []


def footprint(c):
    """the BEV polygon of lib/core.py:289-294: corners 7, 2, 3, 6 in (x, z)"""
    return [(float(c[0, i]), float(c[2, i])) for i in (7, 2, 3, 6)]


def intersection_area(pa, pb):
    """area of the intersection of two convex quadrilaterals (any orientation)"""
    ox = sum(p[0] for p in pa + pb) / 8.0
    oz = sum(p[1] for p in pa + pb) / 8.0
    qa = _ccw([(p[0] - ox, p[1] - oz) for p in pa])
    qb = _ccw([(p[0] - ox, p[1] - oz) for p in pb])
    if _area(qa) == 0 or _area(qb) == 0:
        return 0.0
    pts = [p for p in qa if _inside(p, qb)] + [p for p in qb if _inside(p, qa)]
    for i in range(4):
        for j in range(4):
            # (the crossing of two nearly collinear edges is ill-conditioned and may land anywhere on their lines: a point
            # counts only if it lies in both footprints)
            pts += [p for p in _segment_hits(qa[i], qa[(i + 1) % 4], qb[j], qb[(j + 1) % 4]) if _inside(p, qa) and _inside(p, qb)]
    hull = _hull(pts)
    return _area(hull) if len(hull) >= 3 else 0.0


def aabb_volume(c):
    d = c.max(axis=1) - c.min(axis=1)
    return float(np.prod(d))


def exact_iou(ca, cb, vol=None, volume="aabb"):
    """(iou_bev, iou_3d) of two (3, 8) corner arrays, float64, the reference's formulas (lib/core.py:276-300).  vol None: the sum
    of the corner AABB volumes (volume="aabb", the reference) or of the boxes' own volumes (volume="box")."""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    pa, pb = footprint(ca), footprint(cb)
    aa, ab = abs(_area(pa)), abs(_area(pb))
    if vol is None:
        if volume == "aabb":
            vol = aabb_volume(ca) + aabb_volume(cb)
        else:
            vol = aa * (ca[1].max() - ca[1].min()) + ab * (cb[1].max() - cb[1].min())
    yov = max(0.0, min(ca[1].max(), cb[1].max()) - max(ca[1].min(), cb[1].min()))
    inter = intersection_area(pa, pb)
    with np.errstate(divide="ignore", invalid="ignore"):
        bev = np.float64(inter) / np.float64(ab + aa - inter)
        i3 = np.float64(yov * inter) / np.float64(vol - yov * inter)
    return float(bev), float(i3)


def exact_iou_matrix(ca, cb, volume="aabb"):
    """[M, 3, 8] x [N, 3, 8] -> (iou_bev, iou_3d) [M, N] float64"""
    m, n = len(ca), len(cb)
    bev, i3 = np.empty((m, n)), np.empty((m, n))
    for i in range(m):
        for j in range(n):
            bev[i, j], i3[i, j] = exact_iou(ca[i], cb[j], volume=volume)
    return bev, i3


def checker_matrix(ca, cb, volume="aabb"):
    """exact_iou_matrix for large sets: the polygon step runs only where the footprint AABBs overlap with positive area (elsewhere
    the intersection is empty, I = 0), the formulas run on whole matrices.  ca [M, 3, 8], cb [N, 3, 8] -> (iou_bev, iou_3d) float64."""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    fa, fb = ca[:, :, [7, 2, 3, 6]][:, [0, 2]], cb[:, :, [7, 2, 3, 6]][:, [0, 2]]          # [K, 2, 4] footprints (x, z)

    def area(f):
        x, z = f[:, 0], f[:, 1]
        return 0.5 * np.abs((x * np.roll(z, -1, 1) - np.roll(x, -1, 1) * z).sum(1))

    aa, ab = area(fa), area(fb)
    ya0, ya1, yb0, yb1 = ca[:, 1].min(1), ca[:, 1].max(1), cb[:, 1].min(1), cb[:, 1].max(1)
    if volume == "aabb":
        va, vb = np.prod(ca.max(2) - ca.min(2), 1), np.prod(cb.max(2) - cb.min(2), 1)
    else:
        va, vb = aa * (ya1 - ya0), ab * (yb1 - yb0)
    yov = np.maximum(0.0, np.minimum(ya1[:, None], yb1[None]) - np.maximum(ya0[:, None], yb0[None]))
    ox = (np.maximum(fa[:, 0].min(1)[:, None], fb[:, 0].min(1)[None]) < np.minimum(fa[:, 0].max(1)[:, None], fb[:, 0].max(1)[None]))
    oz = (np.maximum(fa[:, 1].min(1)[:, None], fb[:, 1].min(1)[None]) < np.minimum(fa[:, 1].max(1)[:, None], fb[:, 1].max(1)[None]))
    inter = np.zeros((len(ca), len(cb)))
    for i, j in zip(*np.nonzero(ox & oz)):
        inter[i, j] = intersection_area(footprint(ca[i]), footprint(cb[j]))
    with np.errstate(divide="ignore", invalid="ignore"):
        bev = inter / ((ab[None] + aa[:, None]) - inter)
        i3 = (yov * inter) / ((va[:, None] + vb[None]) - yov * inter)
    return bev, i3


def touching_pair(x, z, w, l, ry):
    """two rotated boxes sharing a long edge bit for bit: b's corners 2, 3 (and 1, 0 above them) ARE a's corners 7, 6 (4, 5)"""
    a = corners(x, 1.0, z, w, 1.5, l, ry)
    b = np.array(a, copy=True)
    d = a[:, 7] - a[:, 2]
    for lo, hi in ((2, 7), (3, 6), (1, 4), (0, 5)):
        b[:, lo] = a[:, hi]
        b[:, hi] = a[:, hi] + d
    return a, b


# ---------------------------------------------------------------------------------------------------------------------------
# analytic cases: (name, corners a, corners b, iou_bev, iou_3d with the boxes' own volumes)
# ---------------------------------------------------------------------------------------------------------------------------
def analytic_cases():
    cases = []
    r2 = math.sqrt(2.0)
    cases.append(("square_vs_45deg", corners(0, 0, 0, 2, 1, 2, 0), corners(0, 0, 0, 2, 1, 2, math.pi / 4), 1 / r2, 1 / r2))
    cases.append(("crossed_2x1", corners(3, 1, 7, 1, 2, 2, 0.3), corners(3, 1, 7, 1, 2, 2, 0.3 + math.pi / 2), 1 / 3, 1 / 3))
    for ry in np.linspace(-math.pi, math.pi, 13):
        a = corners(10, 1.5, 20, 2, 1.5, 4, ry)
        b = corners(10 + math.cos(ry), 1.5, 20 - math.sin(ry), 2, 1.5, 4, ry)     # +1 along the box's own l axis
        cases.append(("shift_along_l_ry%+.3f" % ry, a, b, 0.6, 0.6))
    cases.append(("disjoint", corners(0, 0, 0, 2, 1, 4, 0.4), corners(9, 0, 9, 2, 1, 4, -0.2), 0.0, 0.0))
    # two rotated boxes sharing an edge (b = a moved by its own width along z')
    cases.append(("touching_edge", corners(0, 0, 0, 2, 1, 4, 0.0), corners(0, 0, 2, 2, 1, 4, 0.0), 0.0, 0.0))
    a, b = touching_pair(4.0, 17.0, 1.7, 4.2, 0.83)
    cases.append(("touching_edge_rotated", a, b, 0.0, 0.0))
    cases.append(("nested", corners(5, 1, 5, 4, 2, 6, 0.7), corners(5, 1, 5, 1, 2, 2, 0.2), 2 / 24, 2 / 24))
    cases.append(("identical", corners(-3, 1, 30, 1.6, 1.5, 3.9, 0.0), corners(-3, 1, 30, 1.6, 1.5, 3.9, 0.0), 1.0, 1.0))
    cases.append(("identical_rotated", corners(-3, 1, 30, 1.6, 1.5, 3.9, 1.1), corners(-3, 1, 30, 1.6, 1.5, 3.9, 1.1), 1.0, 1.0))
    cases.append(("y_disjoint", corners(0, 0, 0, 2, 1, 4, 0.5), corners(0, 5, 0, 2, 1, 4, 0.5), 1.0, 0.0))
    return cases


@pytest.mark.parametrize("case", analytic_cases(), ids=lambda c: c[0])
def test_checker_reproduces_analytic_cases(case):
    name, a, b, want_bev, want_3d = case
    bev, i3 = exact_iou(a, b, volume="box")
    assert abs(bev - want_bev) <= 1e-12 and abs(i3 - want_3d) <= 1e-12, (name, bev, i3, want_bev, want_3d)
    # either orientation of either footprint
    bev2, i32 = exact_iou(clockwise(a), b, volume="box")
    assert abs(bev2 - want_bev) <= 1e-12 and abs(i32 - want_3d) <= 1e-12, name


def test_checker_special_cases():
    z = corners(1, 1, 1, 0.0, 1, 0.0, 0.3)
    bev, i3 = exact_iou(z, z, volume="box")
    assert math.isnan(bev) and math.isnan(i3)
    # vol=None on a rotated box against itself: the reference's AABB volumes, iou_3d = A h / (2 V_aabb - A h)
    c = corners(2, 1, 8, 1.6, 1.5, 3.9, 0.6)
    bev, i3 = exact_iou(c, c)
    a, h = 1.6 * 3.9, 1.5
    assert abs(bev - 1) <= 1e-12
    assert abs(i3 - a * h / (2 * aabb_volume(c) - a * h)) <= 1e-12 and i3 < 0.9


def test_checker_matrix_agrees_with_the_pair_loop():
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(5)
    p = synthetic.boxes_3d(rng, 96, clustered=True, per=8).astype(np.float64)
    c = np.stack([corners(*row) for row in p])
    for volume in ("aabb", "box"):
        want = exact_iou_matrix(c[:40], c[40:], volume=volume)
        got = checker_matrix(c[:40], c[40:], volume=volume)
        for w, g in zip(want, got):
            assert np.allclose(w, g, rtol=0, atol=1e-14, equal_nan=True)
        assert (want[0] > 0).sum() > 10


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    from groomed_nms_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared in the header" % name
        assert name in _lib.EXPORTED_SYMBOLS, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "libgroomed_nms_hip.so does not export %s" % name
    assert lib.gnms_abi_version() == 1
    from groomed_nms_amd import overlaps
    assert "iou3d" in overlaps.__all__ and "iou3d_exact_batched" in overlaps.__all__


def test_argument_validation_without_gpu(lib):
    """every check returns -1 before any HIP call; a call with zero pairs returns 0 and launches nothing"""
    fake = ctypes.c_void_p(256 * 1024)            # never dereferenced on the host
    for fn in (lib.gnms_iou3d_exact, lib.gnms_iou3d_exact_from_params):
        assert fn(None, fake, 1, 4, 8, 0, fake, fake, 8, None) == -1                    # null input a
        assert fn(fake, None, 1, 4, 8, 0, fake, fake, 8, None) == -1                    # null input b
        assert fn(fake, fake, 1, 4, 8, 0, None, None, 8, None) == -1                    # both outputs null
        assert b"both NULL" in lib.gnms_last_error()
        assert fn(fake, fake, 1, 4, 8, 0, fake, None, 7, None) == -1                    # ld < N
        assert b"ld" in lib.gnms_last_error()
        for b_, m_, n_ in ((-1, 4, 8), (1, -4, 8), (1, 4, -8)):
            assert fn(fake, fake, b_, m_, n_, 0, fake, fake, 8, None) == -1             # negative sizes
        for mode in (-1, 2, 7):
            assert fn(fake, fake, 1, 4, 8, mode, fake, fake, 8, None) == -1             # volume_mode not in {0, 1}
            assert b"volume_mode" in lib.gnms_last_error()
        assert fn(fake, fake, 0, 4, 8, 0, fake, fake, 8, None) == 0                      # zero pairs
        assert fn(fake, fake, 1, 0, 8, 1, fake, fake, 8, None) == 0
        assert fn(fake, fake, 1, 4, 0, 0, fake, fake, 0, None) == 0
    f = lib.gnms_iou3d_exact_list_f64
    assert f(None, fake, 5, None, fake, fake, None) == -1
    assert f(fake, None, 5, None, fake, fake, None) == -1
    assert f(fake, fake, 5, None, None, None, None) == -1
    assert f(fake, fake, -1, None, fake, fake, None) == -1
    assert f(fake, fake, 0, None, fake, fake, None) == 0
