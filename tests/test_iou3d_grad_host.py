"""d overlap3d / d cuboid on the host: the closed form the HIP kernels evaluate, stated once in float64 NumPy, against
float64 torch autograd of a restatement of the reference's expression from the seven parameters (lib/math_3d.py:364-435,
lib/core.py:305-421, lib/loss/rpn_3d.py:781) and against the reference's own float32 gradients (tests/golden/iou3d_grad.npz); the tie
conventions; the error bound the GPU tests hold the kernels to, checked first on the reference's float32 gradients (a condition on the
reference); the declarations and the argument checks of the new C entries.

`pair_terms3d`, `chain`, `closed_form3d`, `closed_form3d_self`, `layer_reference3d`, `extents_of_corners`, the case builders and
test_iou_grad_host.bound_ratio are what tests/test_iou3d_grad_gpu.py imports.

Two stages, as in DESIGN 3.24.  Stage 2 works on the six axis-aligned extents E = (x0, x1, y0, y1, z0, z1) of either box; stage 1
(`chain`) carries a box's summed extent gradient to (x3d, y3d, z3d, w3d, h3d, l3d, ry3d).  Ties, active clamps and which edge is the
max are decided on the extents the evaluation under comparison SAW: a float32 implementation rounds the corners once (an absolute
error of 2^-24 |coordinate|, which against an intersection extent of a few centimetres is thousands of units in the last place of
that extent), so wherever a float32 result is held to the bound the closed form takes the float32 extents of that result (`ext_a`,
`ext_b`: min / max of its float32 corners, exact operations) and evaluates stage 2 on them in float64; stage 1 uses the parameters.
Against float64 autograd the extents are the float64 ones of the parameters.

The bound (derived, not measured): for gradient element (i, k) with n_i non-zero cotangents,
    |got - f64| <= chain_abs( (n_i + C) * 2^-24 * sum_j |g_ij| * S_ij )          C = 72
S is the two quotient rules with absolute values, per extent,
    S = cI (|dI| U + I (|dvol| + |dI|)) / U^2 + cH ((|dvol| + |dI|) H + U |dH|) / H^2,
chain_abs is stage 1 with absolute values, n_i covers the additions in any order, and C the roundings of ONE term in float32, in units
u = 2^-24, to first order, worst case:
    an extent difference (e, h, a box's length) is one subtraction of given extents: u.  dI = share * pass * (e e): 3u.  I = (e e) e: 5u.
    vol = (l l) l: 5u; vol_a + vol_b: 6u; U = (vol_a + vol_b) - I: absolute 6u (vol_a + vol_b) + 5u I + u U <= 18u U, because
    I <= min(vol) <= U and vol_a + vol_b <= 2 U.  dvol = l l: 3u; dU = dvol - dI: 4u (|dvol| + |dI|).  1 / (U U): 38u.
    dI U: 22u;  I dU: 10u (against I (|dvol| + |dI|));  their difference 1u;  times 1 / U^2: 39u  ->  at most 62u S for the first
    quotient, and no more for the second (H = (h h) h: 5u, dH: 3u, 1 / (H H): 12u);  the sum of the two, the method's factor and the
    cotangent: 2u  ->  64u.  Stage 1: cosf / sinf of the float32 yaw (2u each), a product and a sum per coefficient, the two-term sum
    and the halving: at most 8u against chain_abs  ->  C = 72.
An element whose bound is 0 (no non-zero cotangent, or only terms whose S is 0) must be exactly 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_iou_grad_host import U32, U64, bound_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "iou3d_grad.npz")
C3D = 72
METHOD_FACTORS = {0: (1.0, 0.0), 1: (1.0, 1.0), 2: (0.5, 0.5)}       # (cI, cH): I/U;  I/U - (H - U)/H;  0.5 (1 + that)


# ----------------------------------------------------------------------------------------------------------------------------------
# the derivative of the issue, in float64
# ----------------------------------------------------------------------------------------------------------------------------------
def extents_of(params):
    """params [K, 7] -> E [K, 6] = (x0, x1, y0, y1, z0, z1) in float64: stage 1's forward"""
    p = np.asarray(params, np.float64)
    x, y, z, w, h, l, ry = p.T
    c, s = np.abs(np.cos(ry)), np.abs(np.sin(ry))
    ex, ez = c * l + s * w, s * l + c * w
    return np.stack([x - ex / 2, x + ex / 2, y - h / 2, y + h / 2, z - ez / 2, z + ez / 2], 1)


def extents_of_corners(corners):
    """corners [K, 3, 8] (any float dtype) -> E [K, 6] float64: min / max over the corners, exact"""
    c = np.asarray(corners, np.float64)
    return np.stack([c[:, 0].min(1), c[:, 0].max(1), c[:, 1].min(1), c[:, 1].max(1), c[:, 2].min(1), c[:, 2].max(1)], 1)


def _share(s, o, greater):                                            # ties split evenly
    return np.where(s == o, 0.5, ((s > o) if greater else (s < o)).astype(np.float64))


def _half_at_zero(d):                                                 # torch.max(zeros, d): 1, 1/2 at exactly 0, 0
    return np.where(d > 0, 1.0, np.where(d == 0, 0.5, 0.0))


def pair_terms3d(ea, eb, method=2):
    """ea, eb [K, 6] float64 extents, pair k = (ea[k], eb[k]).  Returns (f [K], d_a [K, 6], d_b [K, 6], S_a [K, 6], S_b [K, 6]): the
    overlap of the method, its derivative w.r.t. the extents of either box, and the two quotient rules with absolute values."""
    ea, eb = np.asarray(ea, np.float64), np.asarray(eb, np.float64)
    ci, ch = METHOD_FACTORS[method]
    e, h, pe, ph = [], [], [], []
    for ax in (0, 1, 2):
        lo_a, hi_a, lo_b, hi_b = ea[:, 2 * ax], ea[:, 2 * ax + 1], eb[:, 2 * ax], eb[:, 2 * ax + 1]
        d = np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b)
        D = np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)
        e.append(np.maximum(d, 0.0))
        h.append(np.maximum(D, 0.0))
        pe.append(_half_at_zero(d) if ax == 1 else (d >= 0).astype(np.float64))      # y: torch.max(zeros, .); x, z: clamp(., 0)
        ph.append(_half_at_zero(D))
    I = e[0] * e[2] * e[1]
    H = h[0] * h[2] * h[1]                                            # (one association throughout: identical boxes give I = U = H to the bit)
    la, lb = ea[:, 1::2] - ea[:, 0::2], eb[:, 1::2] - eb[:, 0::2]
    U = la[:, 0] * la[:, 2] * la[:, 1] + lb[:, 0] * lb[:, 2] * lb[:, 1] - I
    with np.errstate(divide="ignore", invalid="ignore"):              # (a degenerate pair is the reference's 0/0)
        f = I / U if method == 0 else (I / U - (H - U) / H if method == 1 else 0.5 * (1.0 + I / U - (H - U) / H))

    def one(s, o, ls):
        d_i, d_h, d_v = np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)
        for ax in (0, 1, 2):
            others = [k for k in (0, 1, 2) if k != ax]
            pi = pe[ax] * e[others[0]] * e[others[1]]
            pH = ph[ax] * h[others[0]] * h[others[1]]
            av = ls[:, others[0]] * ls[:, others[1]]
            lo, hi = 2 * ax, 2 * ax + 1
            d_i[:, lo] = -_share(s[:, lo], o[:, lo], True) * pi       # the intersection's lower edge is the max of the two
            d_i[:, hi] = _share(s[:, hi], o[:, hi], False) * pi
            d_h[:, lo] = -_share(s[:, lo], o[:, lo], False) * pH      # the hull's lower edge is the min
            d_h[:, hi] = _share(s[:, hi], o[:, hi], True) * pH
            d_v[:, lo], d_v[:, hi] = -av, av
        u, i, hh = U[:, None], I[:, None], H[:, None]
        d_u = d_v - d_i
        with np.errstate(divide="ignore", invalid="ignore"):
            d = ci * (d_i * u - i * d_u) / u ** 2
            S = ci * (np.abs(d_i) * u + i * (np.abs(d_v) + np.abs(d_i))) / u ** 2
            if ch:
                d = d + ch * (d_u * hh - u * d_h) / hh ** 2
                S = S + ch * ((np.abs(d_v) + np.abs(d_i)) * hh + u * np.abs(d_h)) / hh ** 2
        return d, S

    d_a, s_a = one(ea, eb, la)
    d_b, s_b = one(eb, ea, lb)
    return f, d_a, d_b, s_a, s_b


def _sgn(v):
    return np.sign(v)                                                 # sgn 0 = 0: tied corners share the gradient


def chain(params, G):
    """stage 1: G [K, 6] = dL/dE -> dL/d(x, y, z, w, h, l, ry) [K, 7]"""
    p, G = np.asarray(params, np.float64), np.asarray(G, np.float64)
    w, l, ry = p[:, 3], p[:, 5], p[:, 6]
    c, s = np.cos(ry), np.sin(ry)
    gx, gz = G[:, 1] - G[:, 0], G[:, 5] - G[:, 4]
    return np.stack([G[:, 0] + G[:, 1], G[:, 2] + G[:, 3], G[:, 4] + G[:, 5], (np.abs(s) * gx + np.abs(c) * gz) / 2, (G[:, 3] - G[:, 2]) / 2,
                     (np.abs(c) * gx + np.abs(s) * gz) / 2,
                     ((c * _sgn(s) * w - s * _sgn(c) * l) * gx + (c * _sgn(s) * l - s * _sgn(c) * w) * gz) / 2], 1)


def chain_abs(params, A):
    """stage 1 with absolute values: A [K, 6] >= 0 bounds |dL/dE| (or its error) -> the bound on the seven parameters"""
    p, A = np.asarray(params, np.float64), np.asarray(A, np.float64)
    w, l, ry = np.abs(p[:, 3]), np.abs(p[:, 5]), p[:, 6]
    c, s = np.abs(np.cos(ry)), np.abs(np.sin(ry))
    lc, ls = (c != 0), (s != 0)                                      # |sgn|
    ax, az = A[:, 0] + A[:, 1], A[:, 4] + A[:, 5]
    return np.stack([ax, A[:, 2] + A[:, 3], az, (s * ax + c * az) / 2, (A[:, 2] + A[:, 3]) / 2, (c * ax + s * az) / 2,
                     ((c * ls * w + s * lc * l) * ax + (c * ls * l + s * lc * w) * az) / 2], 1)


def _scatter6(idx, vals, n):
    return np.stack([np.bincount(idx, weights=vals[:, k], minlength=n) for k in range(6)], 1) if len(idx) else np.zeros((n, 6))


def closed_form3d(pa, pb, g, method=2, ext_a=None, ext_b=None):
    """pa [M, 7], pb [N, 7], g [M, N] (any float dtype) -> dict(d_a [M, 7], d_b [N, 7], bound_a, bound_b, abs_a, abs_b) in float64.
    ext_a / ext_b: the extents stage 2 is evaluated on (default: the float64 extents of the parameters).  Only the pairs with a
    non-zero cotangent are evaluated: a pair whose cotangent is exactly 0 contributes nothing."""
    pa, pb, g = np.asarray(pa, np.float64), np.asarray(pb, np.float64), np.asarray(g, np.float64)
    ea = extents_of(pa) if ext_a is None else np.asarray(ext_a, np.float64)
    eb = extents_of(pb) if ext_b is None else np.asarray(ext_b, np.float64)
    M, N = len(pa), len(pb)
    i, j = np.nonzero(g)
    gv = g[i, j][:, None]
    _, d_a, d_b, s_a, s_b = pair_terms3d(ea[i], eb[j], method)
    n_a = np.bincount(i, minlength=M)[:, None]
    n_b = np.bincount(j, minlength=N)[:, None]
    return dict(d_a=chain(pa, _scatter6(i, gv * d_a, M)), d_b=chain(pb, _scatter6(j, gv * d_b, N)),
                bound_a=chain_abs(pa, (n_a + C3D) * U32 * _scatter6(i, np.abs(gv) * s_a, M)),
                bound_b=chain_abs(pb, (n_b + C3D) * U32 * _scatter6(j, np.abs(gv) * s_b, N)))


def closed_form3d_self(p, g, method=2, ext=None):
    """overlap(x, x): both roles summed into one gradient; the bound's n_i counts the terms of both roles"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    e = extents_of(p) if ext is None else np.asarray(ext, np.float64)
    n = len(p)
    i, j = np.nonzero(g)
    gv = g[i, j][:, None]
    _, d_a, d_b, s_a, s_b = pair_terms3d(e[i], e[j], method)
    cnt = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n))[:, None]
    return dict(d=chain(p, _scatter6(i, gv * d_a, n) + _scatter6(j, gv * d_b, n)),
                bound=chain_abs(p, (cnt + C3D) * U32 * (_scatter6(i, np.abs(gv) * s_a, n) + _scatter6(j, np.abs(gv) * s_b, n))))


def layer_reference3d(params, grad_iou64, ext=None, cot_tol=True):
    """(dL/dparams3d, its bound) in float64 from a float64 matrix gradient: the closed form of overlap(x, x), method 2, and on top of the
    bound what a float32 matrix gradient may itself be off by -- sum (5e-4 + 1e-3 |g|) |d overlap| over the entries that are non-zero
    (the suite's grad_iou tolerance, carried through stage 1 with absolute values)"""
    p = np.asarray(params, np.float64)
    f = closed_form3d_self(p, grad_iou64, 2, ext)
    bound = f["bound"]
    if cot_tol:
        e = extents_of(p) if ext is None else np.asarray(ext, np.float64)
        i, j = np.nonzero(grad_iou64)
        tol = (5e-4 + 1e-3 * np.abs(grad_iou64[i, j]))[:, None]
        _, d_a, d_b, _, _ = pair_terms3d(e[i], e[j], 2)
        bound = bound + chain_abs(p, _scatter6(i, tol * np.abs(d_a), len(p)) + _scatter6(j, tol * np.abs(d_b), len(p)))
    return f["d"], bound


# ----------------------------------------------------------------------------------------------------------------------------------
# the overlap of every pair in torch operations, from the seven parameters, for autograd to differentiate: what the reference computes,
# written axis by axis.  maximum / minimum of two tensors split the gradient of a tie evenly, clamp passes it at its bound,
# maximum(zeros, .) halves it there, and amax / amin over a box's own corners share it among tied corners (the reference's
# min / max(dim=...) sends it to one of them: the deliberate difference of DESIGN 3.24).
# ----------------------------------------------------------------------------------------------------------------------------------
def torch_extents(p):
    x, y, z, w, h, l, ry = p.unbind(1)
    c, s = torch.cos(ry)[:, None], torch.sin(ry)[:, None]
    bx = torch.stack([-l / 2, l / 2, -l / 2, l / 2], 1)
    bz = torch.stack([-w / 2, -w / 2, w / 2, w / 2], 1)
    cx = c * bx + s * bz + x[:, None]
    cz = -s * bx + c * bz + z[:, None]
    return cx.amin(1), cx.amax(1), y - h / 2, y + h / 2, cz.amin(1), cz.amax(1)


def torch_overlap3d(pa, pb, method=2):
    """pa [M, 7], pb [N, 7] -> [M, N]"""
    a, b = torch_extents(pa), torch_extents(pb)
    zero = torch.zeros((1,), dtype=pa.dtype)
    e, h = [], []
    for ax in (0, 1, 2):
        lo_a, hi_a, lo_b, hi_b = a[2 * ax][:, None], a[2 * ax + 1][:, None], b[2 * ax][None, :], b[2 * ax + 1][None, :]
        d = torch.minimum(hi_a, hi_b) - torch.maximum(lo_a, lo_b)
        e.append(torch.maximum(zero, d) if ax == 1 else d.clamp(min=0))
        h.append(torch.maximum(zero, torch.maximum(hi_a, hi_b) - torch.minimum(lo_a, lo_b)))
    inter = e[0] * e[2] * e[1]
    vol = lambda t: (t[1] - t[0]) * (t[3] - t[2]) * (t[5] - t[4])     # noqa: E731
    union = vol(a)[:, None] + vol(b)[None, :] - inter
    q = inter / union
    if method == 0:
        return q
    hull = h[0] * h[1] * h[2]
    q = q - (hull - union) / hull
    return q if method == 1 else 0.5 * (1.0 + q)


def autograd3d(pa, pb, g, method=2):
    ta = torch.tensor(np.asarray(pa, np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(pb, np.float64), requires_grad=True)
    torch_overlap3d(ta, tb, method).backward(torch.tensor(np.asarray(g, np.float64)))
    return ta.grad.numpy(), tb.grad.numpy()


def autograd3d_self(p, g, method=2):
    t = torch.tensor(np.asarray(p, np.float64), requires_grad=True)
    torch_overlap3d(t, t, method).backward(torch.tensor(np.asarray(g, np.float64)))
    return t.grad.numpy()


# ----------------------------------------------------------------------------------------------------------------------------------
# cases (shared with the GPU tests and the fixture's maker)
# ----------------------------------------------------------------------------------------------------------------------------------
def clustered_pair3d(seed, m, n, per=8):
    """a [m, 7], b [n, 7] fp32 cuboids out of the same clusters (synthetic.boxes_3d), so that a good share of the pairs overlap"""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    both = synthetic.boxes_3d(rng, m + n, clustered=True, per=max(1, min(per, m + n)))
    return np.ascontiguousarray(both[:m]), np.ascontiguousarray(both[m:])


def cotangent3d(seed, m, n, density=1.0):
    rng = np.random.default_rng(seed + 177)
    g = rng.uniform(-1, 2, size=(m, n)).astype(np.float32)
    if density < 1.0:
        g[rng.uniform(size=(m, n)) >= density] = 0.0
    return g


TIE_KINDS = ("identical", "touching_x", "touching_y", "ry0_overlapping", "shared_edges", "degenerate_hull")


def tie_cuboids(seed, k):
    """a, b [6 k, 7] fp32 with ry = 0 and coordinates that are small multiples of 1/4, so that the float32 and the float64 extents are
    the same numbers and every tie is exact: b[q] stands to a[q] as identical / touching in x (d = 0: the clamp passes) / touching in y
    (d = 0: one half) / overlapping with ry = 0 (d ry is the symmetric value, 0) / sharing the lower x, upper y and both z edges /
    a zero-height pair in one plane (hull volume 0: every term of methods 1 and 2 is 0/0 there)."""
    rng = np.random.default_rng(seed)
    n = 6 * k
    q = lambda lo, hi: rng.integers(lo * 4, hi * 4, n).astype(np.float64) / 4     # noqa: E731
    a = np.stack([q(-8, 8), q(0, 3), q(5, 30), q(1, 3) + 0.5, q(1, 3) + 0.5, q(3, 6) + 0.5, np.zeros(n)], 1)   # x y z w h l ry
    b = a.copy()
    kind = np.arange(n) % 6
    t = kind == 1                                                     # b.x0 == a.x1 (extent in x is l at ry = 0)
    b[t, 5] = a[t, 5] + 1.0
    b[t, 0] = a[t, 0] + a[t, 5] / 2 + b[t, 5] / 2
    b[t, 2] = a[t, 2] + 0.25
    t = kind == 2                                                     # b.y0 == a.y1
    b[t, 4] = a[t, 4] + 0.5
    b[t, 1] = a[t, 1] + a[t, 4] / 2 + b[t, 4] / 2
    b[t, 0] = a[t, 0] + 0.25
    t = kind == 3
    b[t, 0] = a[t, 0] + 0.75
    b[t, 1] = a[t, 1] + 0.25
    b[t, 2] = a[t, 2] - 0.25
    b[t, 3] = a[t, 3] + 0.5
    t = kind == 4                                                     # x0 shared (longer b), y1 shared (taller b), z0 and z1 shared
    b[t, 5] = a[t, 5] + 1.0
    b[t, 0] = a[t, 0] + 0.5
    b[t, 4] = a[t, 4] + 1.0
    b[t, 1] = a[t, 1] - 0.5
    t = kind == 5                                                     # both flat, in the same plane: I = 0, H = 0
    a[t, 4] = b[t, 4] = 0.0
    b[t, 0] = a[t, 0] + 0.5
    return a.astype(np.float32), b.astype(np.float32)


# (tag, M, N, density)
HOST_SHAPES3D = [("1x1", 1, 1, 1.0), ("5x7", 5, 7, 1.0), ("64x65", 64, 65, 1.0), ("257x300", 257, 300, 1.0), ("300x257_1pct", 300, 257, 0.01)]


def host_case3d(tag, m, n, density):
    if tag == "1x1":
        a = np.array([[1.0, 1.5, 20.0, 1.6, 1.5, 4.0, 0.3]], np.float32)
        b = np.array([[1.5, 1.3, 20.5, 1.7, 1.6, 3.8, -0.2]], np.float32)
    else:
        a, b = clustered_pair3d(14000 + m + n, m, n)
    return a, b, cotangent3d(m * 31 + n, m, n, density)


# ----------------------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------------------
SCALE64 = 2.0 * U64 / U32     # float64 autograd rounds like any evaluation: the same bound with float64's unit roundoff, for either side


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("case", HOST_SHAPES3D, ids=[c[0] for c in HOST_SHAPES3D])
def test_closed_form_is_float64_autograd(case, method):
    a, b, g = host_case3d(*case)
    f = closed_form3d(a, b, g, method)
    ga, gb = autograd3d(a, b, g, method)
    assert np.isfinite(f["d_a"]).all() and np.isfinite(f["d_b"]).all() and f["d_a"].any()
    assert (np.abs(f["d_a"] - ga) <= SCALE64 * f["bound_a"]).all() and (np.abs(f["d_b"] - gb) <= SCALE64 * f["bound_b"]).all()
    # the overlap itself
    fwd = pair_terms3d(np.repeat(extents_of(a), len(b), 0), np.tile(extents_of(b), (len(a), 1)), method)[0].reshape(len(a), len(b))
    ref = torch_overlap3d(torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64), method).numpy()
    np.testing.assert_allclose(fwd, ref, rtol=0, atol=1e-13)


@pytest.mark.parametrize("n", [1, 41, 300])
def test_self_form_and_its_diagonal(n):
    x, _ = clustered_pair3d(111 + n, n, 1)
    g = np.diag(np.random.default_rng(n).uniform(0.5, 2, n)).astype(np.float32)
    for method in (0, 1, 2):
        f = closed_form3d_self(x, g, method)
        assert not f["d"].any()                                       # identical boxes: exactly 0 in either role, so the diagonal contributes nothing
        assert (np.abs(autograd3d_self(x, g, method)) <= SCALE64 * f["bound"]).all()
    g = cotangent3d(n, n, n)
    f = closed_form3d_self(x, g)
    assert (np.abs(f["d"] - autograd3d_self(x, g)) <= SCALE64 * f["bound"]).all()


@pytest.mark.parametrize("k", [1, 7])
def test_tie_conventions(k):
    a, b = tie_cuboids(5, k)
    assert np.array_equal(extents_of(a), extents_of(a.astype(np.float64)).astype(np.float32))      # the extents are float32 numbers
    kind = np.arange(len(a)) % 6
    sane = kind != 5
    g = cotangent3d(9, len(a), len(b))
    g[~sane, :] = 0.0                                                 # a pair with a flat box is 0/0 in every method: its cotangent must be 0
    g[:, ~sane] = 0.0
    for method in (0, 1, 2):
        f = closed_form3d(a, b, g, method)
        ga, gb = autograd3d(a, b, g, method)
        assert np.isfinite(f["d_a"]).all() and np.isfinite(f["d_b"]).all()
        assert not f["d_a"][~sane].any() and not f["d_b"][~sane].any()
        # (autograd multiplies the zero cotangent into the degenerate pairs' NaN: compare the boxes it can speak about; and it reaches
        # the symmetric d ry = 0 through the tied corners' shares, which cancel to its roundoff only: that column is held to the bound
        # the same boxes have a hair off ry = 0, where every corner counts)
        off_a, off_b = a.astype(np.float64), b.astype(np.float64)
        off_a[:, 6] = off_b[:, 6] = 1e-300
        off = closed_form3d(off_a, off_b, g, method)
        bound_a, bound_b = f["bound_a"].copy(), f["bound_b"].copy()
        bound_a[:, 6], bound_b[:, 6] = off["bound_a"][:, 6], off["bound_b"][:, 6]
        assert (np.abs(f["d_a"] - ga)[sane] <= SCALE64 * bound_a[sane]).all()
        assert (np.abs(f["d_b"] - gb)[sane] <= SCALE64 * bound_b[sane]).all()
        assert not f["d_a"][:, 6].any() and not f["d_b"][:, 6].any()  # ry = 0: the tied corners share, d ry is the symmetric value
    # the pairs themselves, one at a time (method 0, so that each convention shows alone)
    ea, eb = extents_of(a), extents_of(b)
    q, d_a, d_b, _, _ = pair_terms3d(ea, eb, 0)
    assert (q[kind == 0] == 1.0).all() and (q[(kind == 1) | (kind == 2)] == 0.0).all()
    assert not d_a[kind == 0].any() and not d_b[kind == 0].any()      # identical: exactly 0 in each role
    vol = lambda e: (e[:, 1] - e[:, 0]) * (e[:, 3] - e[:, 2]) * (e[:, 5] - e[:, 4])    # noqa: E731
    un = vol(ea) + vol(eb)

    def ext(t, ax):
        return np.minimum(ea[t, 2 * ax + 1], eb[t, 2 * ax + 1]) - np.maximum(ea[t, 2 * ax], eb[t, 2 * ax])
    t = kind == 1                                                     # touching in x: the clamp passes, factor 1
    assert (ext(t, 1) > 0).all() and (ext(t, 2) > 0).all()
    np.testing.assert_allclose(d_a[t, 1], ext(t, 1) * ext(t, 2) / un[t], rtol=1e-14)
    np.testing.assert_allclose(d_b[t, 0], -ext(t, 1) * ext(t, 2) / un[t], rtol=1e-14)
    t = kind == 2                                                     # touching in y: torch.max(zeros, .), factor 1/2
    np.testing.assert_allclose(d_a[t, 3], 0.5 * ext(t, 0) * ext(t, 2) / un[t], rtol=1e-14)
    np.testing.assert_allclose(d_b[t, 2], -0.5 * ext(t, 0) * ext(t, 2) / un[t], rtol=1e-14)
    # degenerate hull: H = 0 under a non-zero cotangent is the reference's 0/0
    with np.errstate(all="ignore"):
        bad = pair_terms3d(ea[kind == 5], eb[kind == 5], 2)
    assert not np.isfinite(bad[1]).all()


def test_ry_zero_is_the_mean_of_the_one_sided_derivatives():
    """sgn 0 = 0: at ry = 0 the closed form's d ry is the mean of the derivatives just left and right of 0 (the reference picks one
    tied corner, an arbitrary non-zero value)"""
    a, b = tie_cuboids(3, 4)
    keep = (np.arange(len(a)) % 6) == 3
    a, b = a[keep].astype(np.float64), b[keep].astype(np.float64)
    g = cotangent3d(2, len(a), len(b))
    at0 = closed_form3d(a, b, g)["d_a"][:, 6]
    assert not at0.any()
    eps = 1e-7
    lo, hi = a.copy(), a.copy()
    lo[:, 6], hi[:, 6] = -eps, eps
    sides = 0.5 * (closed_form3d(lo, b, g)["d_a"][:, 6] + closed_form3d(hi, b, g)["d_a"][:, 6])
    one_sided = closed_form3d(hi, b, g)["d_a"][:, 6]
    assert np.abs(one_sided).max() > 1e-3 and np.abs(sides).max() < 1e-5 * np.abs(one_sided).max()


def test_golden_overlap_gradients_are_the_closed_form():
    """the reference's own float32 iou3d_approximate(get_corners_of_cuboid(...)).backward(cotangent), recorded by
    tests/golden/make_iou3d_grad_golden.py with the float32 extents its corners had"""
    z = np.load(GOLDEN)
    tags = [str(t) for t in z["overlap_cases"]]
    assert len(tags) >= 5 and any("self" in t for t in tags) and sum("method" in t for t in tags) == 2
    for t in tags:
        g, method = z["overlap/%s/cotangent" % t], int(z["overlap/%s/method" % t])
        if "self" in t:
            f = closed_form3d_self(z["overlap/%s/a" % t], g, method, ext=z["overlap/%s/ext_a" % t])
            r = bound_ratio(z["overlap/%s/grad_a" % t], f["d"], f["bound"])
        else:
            f = closed_form3d(z["overlap/%s/a" % t], z["overlap/%s/b" % t], g, method, z["overlap/%s/ext_a" % t], z["overlap/%s/ext_b" % t])
            r = max(bound_ratio(z["overlap/%s/grad_a" % t], f["d_a"], f["bound_a"]), bound_ratio(z["overlap/%s/grad_b" % t], f["d_b"], f["bound_b"]))
        print("reference float32 / bound  %-22s %.3f" % (t, r))
        assert r <= 1.0, t


def test_golden_layer_cuboid_gradients_are_grad_iou_contracted_by_the_closed_form():
    """the reference's differentiable_nms(scores, 0.5 (1 + iou3d_approximate(corners(params)))) with params.requires_grad, float32 on the
    CPU: params.grad equals the float64 layer's matrix gradient (test_grad_iou_host.f64_layer) contracted with the closed form, to the
    bound plus -- where the 2D tests add it, every mode but masked-linear -- the suite's grad_iou tolerance"""
    from oracle import oracle as O
    from test_grad_iou_host import DEFAULTS, f64_layer, left_out
    z = np.load(GOLDEN)
    tags = [str(t) for t in z["layer_cases"]]
    assert sorted(tags) == sorted(["default", "cap5", "unmasked", "ungrouped", "sigmoidal"])
    for t in tags:
        p, scores, w = z["layer/%s/params" % t], z["layer/%s/scores" % t], z["layer/%s/weights" % t]
        kw = {k[len("layer/%s/kw/" % t):]: z[k].item() for k in z.files if k.startswith("layer/%s/kw/" % t)}
        # (the float32 matrix, for the grouping: the oracle's; the maker keeps every overlap 8 eps away from the threshold)
        corners = O.corners_of_cuboid(p)
        m = (np.float32(0.5) * (np.float32(1.0) + O.iou3d_approximate(corners, corners, True)[1])).astype(np.float32)
        f = f64_layer(O, scores, m, w, **kw)
        n_und, skip = left_out(f)
        assert n_und == 0, t
        k = dict(DEFAULTS)
        k.update(kw)
        masked_linear = k["group_boxes"] and k["mask_group_boxes"] and k["pruning_method"] == "linear"
        ref, bound = layer_reference3d(p, f["grad_iou"], ext=z["layer/%s/ext" % t], cot_tol=not masked_linear)
        r = bound_ratio(z["layer/%s/params_grad" % t], ref, bound)
        print("reference float32 layer / bound  %-10s %.3f" % (t, r))
        assert r <= 1.0, t


def test_header_and_ctypes_declare_the_new_entries():
    from groomed_nms_amd import _lib
    text = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gnms_iou3d_backward", "gnms_iou3d_backward_workspace_bytes", "gnms_backward_cuboids", "gnms_backward_cuboids_scratch_bytes",
                 "gnms_backward_cuboids_reads"):
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in the header" % name
        assert name in _lib.EXPORTED_SYMBOLS, "%s has no ctypes signature" % name


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def _host(n):
    return (ctypes.c_float * max(n, 4))()


def test_iou3d_backward_argument_checks_run_before_any_launch(lib):
    """host pointers throughout: every call must fail in the checks (or be an empty problem), never reach a launch"""
    a, b, g, da, db = _host(64), _host(64), _host(256), _host(64), _host(64)
    ws = _host(1 << 16)
    big = 4 << 16
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)                     # noqa: E731
    call = lambda *args: lib.gnms_iou3d_backward(*args)               # noqa: E731
    assert call(p(a), p(b), p(g), -1, 4, 4, 4, 2, p(da), p(db), p(ws), big, None) == -1 and b"negative" in lib.gnms_last_error()
    assert call(p(a), p(b), p(g), 1, -4, 4, 4, 2, p(da), p(db), p(ws), big, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, -4, 4, 2, p(da), p(db), p(ws), big, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, 4, 3, 2, p(da), p(db), p(ws), big, None) == -1 and b"ld" in lib.gnms_last_error()
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, 3, p(da), p(db), p(ws), big, None) == -1 and b"method" in lib.gnms_last_error()
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, -1, p(da), p(db), p(ws), big, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, 2, None, None, p(ws), big, None) == -1 and b"both outputs" in lib.gnms_last_error()
    assert call(p(a), None, p(g), 1, 4, 5, 5, 2, p(da), None, p(ws), big, None) == -1         # params_b NULL needs M == N
    assert call(p(a), None, p(g), 1, 4, 4, 4, 2, p(da), p(db), p(ws), big, None) == -1        # ... and d_params_b NULL
    assert call(p(a), None, p(g), 1, 4, 4, 4, 2, None, p(db), p(ws), big, None) == -1         # ... and d_params_a given
    assert call(None, p(b), p(g), 1, 4, 4, 4, 2, p(da), p(db), p(ws), big, None) == -1
    assert call(p(a), p(b), None, 1, 4, 4, 4, 2, p(da), p(db), p(ws), big, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, 2, p(da), p(db), None, big, None) == -1 and b"workspace" in lib.gnms_last_error()
    aligned = ctypes.c_void_p(256 * 1024)
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, 2, p(da), p(db), ctypes.c_void_p(256 * 1024 + 64), big, None) == -1   # misaligned
    need = lib.gnms_iou3d_backward_workspace_bytes(1, 4, 4)
    assert need > 0 and need % 256 == 0 and lib.gnms_iou3d_backward_workspace_bytes(0, 4, 4) == 0
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, 2, p(da), p(db), aligned, need - 1, None) == -4   # GNMS_ERR_WORKSPACE
    assert call(p(a), p(b), p(g), 0, 4, 4, 4, 2, p(da), p(db), None, 0, None) == 0              # an empty batch is a success
    # the records and the slabs are a fraction of the matrix: a unit is at least 32 rows x 128 columns and leaves 24 bytes per row and
    # per column, so at most 24 / (128 * 4) + 24 / (32 * 4) of the matrix's bytes, plus 32 bytes per box
    matrix = 8 * 4096 * 4096 * 4
    assert lib.gnms_iou3d_backward_workspace_bytes(8, 4096, 4096) <= matrix * 3 // 64 + matrix * 3 // 16 + 2 * 8 * 4096 * 32 + 1024


def test_backward_cuboids_argument_checks_and_reads_table(lib):
    from groomed_nms_amd._lib import GnmsParams
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    gp, px, sc, gs, gb = _host(8), _host(56), _host(8), _host(8), _host(56)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)                     # noqa: E731
    big = 1 << 30
    fake_ws = ctypes.c_void_p(256 * 4096)
    call = lambda *args: lib.gnms_backward_cuboids(*args)             # noqa: E731
    assert call(p(gp), p(px), p(sc), -1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(px), p(sc), 1, -8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 7, 0, None, 0, fake_ws, big, None) == -1   # ld < N
    assert b"ld" in lib.gnms_last_error()
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), None, None, None, 8, 0, None, 0, fake_ws, big, None) == -1     # both outputs NULL
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), None, None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), None, p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 7, None, 0, fake_ws, big, None) == -1   # unknown route
    assert b"route" in lib.gnms_last_error()
    assert call(p(gp), p(px), p(sc), 1, 8, None, None, p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, None, big, None) == -1      # workspace NULL
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, 16, None) == -4    # ... too small
    # the dense route asks for its scratch before anything runs
    assert lib.gnms_backward_cuboids_scratch_bytes(1, 8, 8, ctypes.byref(P), 0, 0) == 0         # default mode: the sparse route, no scratch
    need = lib.gnms_backward_cuboids_scratch_bytes(1, 8, 8, ctypes.byref(P), 0, 1)
    assert need >= 2 * 8 * 8 * 4 and need > lib.gnms_backward_cuboids_scratch_bytes(1, 8, 8, ctypes.byref(P), 1, 1) > 0
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 1, None, 0, fake_ws, big, None) == -1   # scratch NULL
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 1, ctypes.c_void_p(256 * 4096 + 16), need, fake_ws, big,
                None) == -1                                           # ... misaligned
    assert call(p(gp), p(px), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 1, fake_ws, need - 1, fake_ws, big, None) == -4
    assert call(p(gp), p(px), p(sc), 0, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, None, 0, None) == 0         # an empty batch

    # what a binding must keep alive: READS_MATRIX = 1, READS_BOXES = 2; never COPY_BOXES (8), whatever the pointer's alignment
    def mode(**kw):
        q = GnmsParams()
        lib.gnms_default_params(ctypes.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    AUTO, DENSE = 0, 1
    table = [(mode(), AUTO, 2), (mode(), DENSE, 3), (mode(group_size=5), AUTO, 2), (mode(pruning_method=1), AUTO, 2),
             (mode(mask_group_boxes=0), AUTO, 3), (mode(group_boxes=0), AUTO, 3), (mode(return_sorted_prob=1), AUTO, 3),
             (mode(presorted=1), AUTO, 3), (mode(group_boxes=0), DENSE, 3)]
    for q, route, want in table:
        for ptr_ in (ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)):
            assert lib.gnms_backward_cuboids_reads(ctypes.byref(q), ptr_, route) == want
    assert lib.gnms_backward_cuboids_reads(None, ctypes.c_void_p(4096), AUTO) == -1 and b"gnms_backward_cuboids_reads" in lib.gnms_last_error()
    assert lib.gnms_backward_cuboids_reads(ctypes.byref(P), None, AUTO) == -1
    assert lib.gnms_backward_cuboids_reads(ctypes.byref(P), ctypes.c_void_p(4096), 2) == -1
    assert lib.gnms_backward_cuboids_reads(ctypes.byref(P), ctypes.c_void_p(4096), -1) == -1
