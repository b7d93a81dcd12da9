"""dIoU/dbox on the host: the closed form the HIP kernels evaluate, stated once in float64 NumPy, against float64 torch
autograd of a restatement of the reference's expression (lib/core.py:210-218, 499-508) and against the reference's own float32
gradients (tests/golden/iou_grad.npz); the tie conventions; the error bound the GPU tests hold the kernels to, checked first on
torch's float32 autograd (a condition on the reference); the declarations and the argument checks of the new C entries.

`closed_form`, `closed_form_self`, `layer_reference`, `bound_ratio` and the case builders are what tests/test_iou_grad_gpu.py imports.

The bound (derived, not measured): for gradient element (i, k) with n_i non-zero cotangents,
    |got - f64| <= (n_i + 16) * 2^-24 * sum_j |g_ij| * S_ijk,     S = (|d inter| union + inter (|d area| + |d inter|)) / union^2
S is the quotient rule with absolute values, 16 covers the roundings of one term, n_i the additions in any order; an element whose
bound is 0 (no non-zero cotangent, or only terms whose S is 0) must be exactly 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "iou_grad.npz")
U32 = 2.0 ** -24                 # unit roundoff of float32
U64 = 2.0 ** -53


# ----------------------------------------------------------------------------------------------------------------------------------
# section 1 of the issue, in float64, pair by pair
# ----------------------------------------------------------------------------------------------------------------------------------
def pair_terms(a, b):
    """a, b [K, 4] float64 = (x1, y1, x2, y2), pair k = (a[k], b[k]).  Returns (iou [K], d_a [K, 4], d_b [K, 4], S_a [K, 4], S_b [K, 4]):
    the IoU, its derivative w.r.t. the coordinates of either box, and the quotient rule with absolute values."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ext, on = [], []
    for ax in (0, 1):
        d = np.minimum(a[:, 2 + ax], b[:, 2 + ax]) - np.maximum(a[:, ax], b[:, ax])
        ext.append(np.maximum(d, 0.0))
        on.append((d >= 0).astype(np.float64))                        # the clamp passes the gradient at 0
    w, h = ext
    inter = w * h
    sa = a[:, 2:] - a[:, :2]
    sb = b[:, 2:] - b[:, :2]
    union = sa[:, 0] * sa[:, 1] + sb[:, 0] * sb[:, 1] - inter

    def share(s, o, upper):                                           # ties split evenly
        return np.where(s == o, 0.5, ((s < o) if upper else (s > o)).astype(np.float64))

    def one(s, o, size):
        other = (h * on[0], w * on[1])                                # d inter / d(an x coordinate) carries h, a y coordinate w
        d_inter = np.stack([-share(s[:, 0], o[:, 0], False) * other[0], -share(s[:, 1], o[:, 1], False) * other[1],
                            share(s[:, 2], o[:, 2], True) * other[0], share(s[:, 3], o[:, 3], True) * other[1]], 1)
        d_area = np.stack([-size[:, 1], -size[:, 0], size[:, 1], size[:, 0]], 1)
        u, i = union[:, None], inter[:, None]
        return (d_inter * u - i * (d_area - d_inter)) / u ** 2, (np.abs(d_inter) * u + i * (np.abs(d_area) + np.abs(d_inter))) / u ** 2

    d_a, s_a = one(a, b, sa)
    d_b, s_b = one(b, a, sb)
    return inter / union, d_a, d_b, s_a, s_b


def _scatter(idx, vals, n):
    return np.stack([np.bincount(idx, weights=vals[:, k], minlength=n) for k in range(4)], 1) if len(idx) else np.zeros((n, 4))


def closed_form(a, b, g):
    """a [M, 4], b [N, 4], g [M, N] (any float dtype) -> dict(d_a [M, 4], d_b [N, 4], bound_a, bound_b) in float64.  Only the pairs
    with a non-zero cotangent are evaluated: a pair whose cotangent is exactly 0 contributes nothing."""
    a, b, g = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(g, np.float64)
    M, N = len(a), len(b)
    i, j = np.nonzero(g)
    gv = g[i, j][:, None]
    _, d_a, d_b, s_a, s_b = pair_terms(a[i], b[j])
    n_a = np.bincount(i, minlength=M)[:, None]
    n_b = np.bincount(j, minlength=N)[:, None]
    return dict(d_a=_scatter(i, gv * d_a, M), d_b=_scatter(j, gv * d_b, N),
                bound_a=(n_a + 16) * U32 * _scatter(i, np.abs(gv) * s_a, M), bound_b=(n_b + 16) * U32 * _scatter(j, np.abs(gv) * s_b, N),
                absdiou_a=_scatter(i, np.abs(d_a), M), absdiou_b=_scatter(j, np.abs(d_b), N))


def closed_form_self(x, g):
    """iou(x, x): both roles summed into one gradient; the bound's n_i counts the terms of both roles"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    n = len(x)
    i, j = np.nonzero(g)
    gv = g[i, j][:, None]
    _, d_a, d_b, s_a, s_b = pair_terms(x[i], x[j])
    cnt = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n))[:, None]
    return dict(d=_scatter(i, gv * d_a, n) + _scatter(j, gv * d_b, n),
                bound=(cnt + 16) * U32 * (_scatter(i, np.abs(gv) * s_a, n) + _scatter(j, np.abs(gv) * s_b, n)))


def bound_ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements with a positive bound; elements whose bound is 0 must be exactly 0"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    zero = bound == 0
    assert not got[zero].any(), "an element with no contributing term is not exactly 0"
    err = np.abs(got - ref)[~zero]
    return float((err / bound[~zero]).max()) if err.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# the IoU of every pair in torch operations, for autograd to differentiate: what the reference computes (lib/core.py:210-218, 499-508),
# written axis by axis.  maximum / minimum of two tensors split the gradient of a tie evenly and clamp passes it at its bound, which
# are the conventions the closed form above states.
# ----------------------------------------------------------------------------------------------------------------------------------
def torch_iou(rows, cols):
    """rows [M, 4], cols [N, 4] -> [M, N]"""
    rx1, ry1, rx2, ry2 = (rows[:, k, None] for k in range(4))
    cx1, cy1, cx2, cy2 = (cols[None, :, k] for k in range(4))
    w = (torch.minimum(rx2, cx2) - torch.maximum(rx1, cx1)).clamp(min=0)
    h = (torch.minimum(ry2, cy2) - torch.maximum(ry1, cy1)).clamp(min=0)
    overlap = w * h
    return overlap / ((rx2 - rx1) * (ry2 - ry1) + (cx2 - cx1) * (cy2 - cy1) - overlap)


def autograd(a, b, g, dtype):
    ta = torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    tb = torch.tensor(np.asarray(b), dtype=dtype, requires_grad=True)
    torch_iou(ta, tb).backward(torch.tensor(np.asarray(g), dtype=dtype))
    return ta.grad.numpy(), tb.grad.numpy()


def autograd_self(x, g, dtype):
    tx = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    torch_iou(tx, tx).backward(torch.tensor(np.asarray(g), dtype=dtype))
    return tx.grad.numpy()


# ----------------------------------------------------------------------------------------------------------------------------------
# cases (shared with the GPU tests)
# ----------------------------------------------------------------------------------------------------------------------------------
def clustered_pair(seed, m, n, per=8):
    """a [m, 4], b [n, 4] fp32 out of the same clusters, so that a good share of the pairs overlap"""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    both = synthetic.clustered_boxes_2d(rng, m + n, max(1, min(per, m + n)))
    both = both[rng.permutation(m + n)]
    return np.ascontiguousarray(both[:m]), np.ascontiguousarray(both[m:])


def tie_boxes(seed, k):
    """a, b [5 k, 4] fp32 with integer-valued pixel coordinates: b[q] stands to a[q] as identical / touching in x (d = 0) / sharing
    the left edge / sharing the top and right edges / touching at a corner.  Coordinates repeat ACROSS pairs too (few distinct
    integers), so the rectangular matrix is full of ties."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(0, 40, 5 * k).astype(np.float64)
    y1 = rng.integers(0, 40, 5 * k).astype(np.float64)
    w = rng.integers(4, 24, 5 * k).astype(np.float64)
    h = rng.integers(4, 24, 5 * k).astype(np.float64)
    a = np.stack([x1, y1, x1 + w, y1 + h], 1)
    b = a.copy()
    kind = np.arange(5 * k) % 5
    t = kind == 1
    b[t] = np.stack([a[t, 2], a[t, 1] + 1, a[t, 2] + 7, a[t, 3] + 2], 1)                 # touching: b.x1 == a.x2
    t = kind == 2
    b[t] = np.stack([a[t, 0], a[t, 1] + 2, a[t, 2] + 3, a[t, 3] + 5], 1)                 # the left edge shared
    t = kind == 3
    b[t] = np.stack([a[t, 0] + 1, a[t, 1] - 3, a[t, 2], a[t, 3]], 1)                     # the right and the lower edge shared
    t = kind == 4
    b[t] = np.stack([a[t, 2], a[t, 3], a[t, 2] + 5, a[t, 3] + 6], 1)                     # touching at a corner: d = 0 on both axes
    return a.astype(np.float32), b.astype(np.float32)


def cotangent(seed, m, n, density=1.0):
    rng = np.random.default_rng(seed + 77)
    g = rng.uniform(-1, 2, size=(m, n)).astype(np.float32)
    if density < 1.0:
        g[rng.uniform(size=(m, n)) >= density] = 0.0
    return g


# (tag, M, N, density): seven shapes from 1 x 1 to 1100 x 1100, dense and 1 %-sparse
HOST_SHAPES = [("1x1", 1, 1, 1.0), ("5x7", 5, 7, 1.0), ("64x65", 64, 65, 1.0), ("257x300", 257, 300, 1.0), ("500x500", 500, 500, 1.0),
               ("500x500_1pct", 500, 500, 0.01), ("1100x1100_1pct", 1100, 1100, 0.01), ("1100x1100", 1100, 1100, 1.0)]


def host_case(tag, m, n, density):
    if tag == "1x1":
        a = np.array([[10, 20, 50, 80]], np.float32)
        b = np.array([[30, 10, 70, 60]], np.float32)
    else:
        a, b = clustered_pair(4000 + m + n, m, n)
    return a, b, cotangent(m * 31 + n, m, n, density)


# ----------------------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HOST_SHAPES, ids=[c[0] for c in HOST_SHAPES])
def test_closed_form_is_float64_autograd_and_bounds_float32_autograd(case):
    a, b, g = host_case(*case)
    f = closed_form(a, b, g)
    ga, gb = autograd(a.astype(np.float64), b.astype(np.float64), g.astype(np.float64), torch.float64)
    # float64 autograd rounds like any evaluation: the same bound with float64's unit roundoff, for either side of the comparison
    scale = 2.0 * U64 / U32
    assert (np.abs(f["d_a"] - ga) <= scale * f["bound_a"]).all() and (np.abs(f["d_b"] - gb) <= scale * f["bound_b"]).all()
    # a condition on the reference: its float32 autograd stays within the bound the kernels are held to
    ga32, gb32 = autograd(a, b, g, torch.float32)
    ra, rb = bound_ratio(ga32, f["d_a"], f["bound_a"]), bound_ratio(gb32, f["d_b"], f["bound_b"])
    print("torch float32 autograd / bound  %-16s d_a %.3f  d_b %.3f" % (case[0], ra, rb))
    assert ra <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("k", [1, 13])
def test_ties_split_evenly_and_the_clamp_passes_at_zero(k):
    a, b = tie_boxes(5, k)
    g = cotangent(9, len(a), len(b))
    f = closed_form(a, b, g)
    ga, gb = autograd(a.astype(np.float64), b.astype(np.float64), g.astype(np.float64), torch.float64)
    scale = 2.0 * U64 / U32
    assert (np.abs(f["d_a"] - ga) <= scale * f["bound_a"]).all() and (np.abs(f["d_b"] - gb) <= scale * f["bound_b"]).all()
    # the pairs themselves, one at a time
    iou, d_a, d_b, _, _ = pair_terms(a, b)
    kind = np.arange(len(a)) % 5
    assert (iou[kind == 0] == 1.0).all() and (iou[(kind == 1) | (kind == 4)] == 0.0).all()
    # identical boxes: inter = union = area and every edge is tied, so half of d inter cancels half of d area in either role, exactly
    assert not d_a[kind == 0].any() and not d_b[kind == 0].any()
    # touching in x, d = 0: inter = 0 but the clamp passes, so the x coordinates that form d see h / union
    t = kind == 1
    hh = np.minimum(a[t, 3], b[t, 3]).astype(np.float64) - np.maximum(a[t, 1], b[t, 1])
    un = ((a[t, 2] - a[t, 0]) * (a[t, 3] - a[t, 1]) + (b[t, 2] - b[t, 0]) * (b[t, 3] - b[t, 1])).astype(np.float64)
    assert np.allclose(d_a[t, 2], hh / un, rtol=1e-15, atol=0) and np.allclose(d_b[t, 0], -hh / un, rtol=1e-15, atol=0)
    assert not d_a[t][:, [0, 1, 3]].any() and not d_b[t][:, [1, 2, 3]].any()
    assert not d_a[kind == 4].any() and not d_b[kind == 4].any()                         # a corner: w = h = 0 kills both


@pytest.mark.parametrize("n", [1, 37, 300])
def test_self_pairs_of_iou_x_x_are_exactly_zero(n):
    x, _ = clustered_pair(11 + n, n, 1)
    g = np.diag(np.random.default_rng(n).uniform(0.5, 2, n)).astype(np.float32)
    f = closed_form_self(x, g)
    assert not f["d"].any()                                           # the tie split makes a self pair's derivative exactly 0 in the closed form
    # (autograd reaches the same 0 through several rounded terms that cancel: to its own roundoff only)
    assert (np.abs(autograd_self(x.astype(np.float64), g.astype(np.float64), torch.float64)) <= 2.0 * U64 / U32 * f["bound"]).all()
    g = cotangent(n, n, n)
    f = closed_form_self(x, g)
    ref = autograd_self(x.astype(np.float64), g.astype(np.float64), torch.float64)
    assert (np.abs(f["d"] - ref) <= 2.0 * U64 / U32 * f["bound"]).all()
    assert bound_ratio(autograd_self(x, g, torch.float32), f["d"], f["bound"]) <= 1.0


def test_golden_iou_gradients_are_the_closed_form():
    """the reference's own float32 lib.core.iou(a, b).backward(cotangent), recorded by tests/golden/make_iou_grad_golden.py"""
    z = np.load(GOLDEN)
    tags = [str(t) for t in z["iou_cases"]]
    assert len(tags) >= 4 and any("self" in t for t in tags) and any("ties" in t for t in tags)
    for t in tags:
        g = z["iou/%s/cotangent" % t]
        if "self" in t:
            f = closed_form_self(z["iou/%s/a" % t], g)
            r = bound_ratio(z["iou/%s/grad_a" % t], f["d"], f["bound"])
        else:
            f = closed_form(z["iou/%s/a" % t], z["iou/%s/b" % t], g)
            r = max(bound_ratio(z["iou/%s/grad_a" % t], f["d_a"], f["bound_a"]), bound_ratio(z["iou/%s/grad_b" % t], f["d_b"], f["bound_b"]))
        print("reference float32 / bound  %-12s %.3f" % (t, r))
        assert r <= 1.0, t


def test_golden_layer_box_gradients_are_grad_iou_contracted_by_the_closed_form():
    """the reference's differentiable_nms(scores, iou(boxes, boxes)) with boxes.requires_grad, float32 on the CPU: boxes.grad equals the
    float64 layer's matrix gradient (test_grad_iou_host.f64_layer) contracted with the closed form, to the bound plus what the
    reference's own float32 matrix gradient may differ by (5e-4 + 1e-3 |g| per entry, the suite's grad_iou tolerance)"""
    from oracle import oracle as O
    from test_grad_iou_host import f64_layer, left_out
    z = np.load(GOLDEN)
    tags = [str(t) for t in z["layer_cases"]]
    assert sorted(tags) == sorted(["default", "cap5", "unmasked", "ungrouped", "sigmoidal"])
    for t in tags:
        boxes, scores, w = z["layer/%s/boxes" % t], z["layer/%s/scores" % t], z["layer/%s/weights" % t]
        kw = {k[len("layer/%s/kw/" % t):]: z[k].item() for k in z.files if k.startswith("layer/%s/kw/" % t)}
        m = O.iou2d(boxes, boxes)
        f = f64_layer(O, scores, m, w, **kw)
        n_und, skip = left_out(f)
        assert n_und == 0, t
        ref, bound = layer_reference(boxes, f["grad_iou"])
        r = bound_ratio(z["layer/%s/boxes_grad" % t], ref, bound)
        print("reference float32 layer / bound  %-10s %.3f" % (t, r))
        assert r <= 1.0, t


def layer_reference(boxes, grad_iou64, cot_tol=True):
    """(dL/dboxes, its bound) in float64 from a float64 matrix gradient: the closed form of iou(x, x), and on top of the bound what
    a float32 matrix gradient may itself be off by -- sum (5e-4 + 1e-3 |g|) |dIoU| over the entries that are non-zero"""
    x = np.asarray(boxes, np.float64)
    f = closed_form_self(x, grad_iou64)
    bound = f["bound"]
    if cot_tol:
        i, j = np.nonzero(grad_iou64)
        tol = (5e-4 + 1e-3 * np.abs(grad_iou64[i, j]))[:, None]
        _, d_a, d_b, _, _ = pair_terms(x[i], x[j])
        bound = bound + _scatter(i, tol * np.abs(d_a), len(x)) + _scatter(j, tol * np.abs(d_b), len(x))
    return f["d"], bound


def f64_unmasked_by_blocks(O, scores, iou, w, **kw):
    """test_grad_iou_host.f64_layer for unmasked groups, group by group: M is block diagonal there, so each group's
    inverse(I_g + P_g) s_g is differentiated on its own block.  The same mathematics and the same fields; f64_layer rebuilds the N x N
    matrix once per group, which at N = 4160 takes half a minute (pinned against it below at a size where both are quick)."""
    from test_grad_iou_host import DEFAULTS, _prune64
    k = dict(DEFAULTS)
    k.update(kw)
    assert k["group_boxes"] and not k["mask_group_boxes"] and not k["return_sorted_prob"]
    thr, temp, vthr = (float(np.float32(k[x])) for x in ("nms_threshold", "temperature", "valid_box_prob_threshold"))
    n = len(scores)
    order = np.asarray(O.argsort_desc(scores))
    s64 = np.asarray(scores, np.float64)[order]
    m32 = np.ascontiguousarray(np.asarray(iou, np.float32)[np.ix_(order, order)])
    groups = [np.asarray(g) for g in O.get_groups(m32, k["nms_threshold"], np.ascontiguousarray(np.asarray(scores, np.float32)[order]),
                                                  k["group_size"]) if len(g)]
    w64 = np.asarray(w, np.float64)
    pre = np.zeros(n)
    grad_iou = np.zeros((n, n))
    grad_scores = np.zeros(n)
    for g in groups:
        x = torch.tensor(m32[np.ix_(g, g)].astype(np.float64), requires_grad=True)
        s = torch.tensor(s64[g], requires_grad=True)
        p = torch.linalg.inv(torch.eye(len(g), dtype=torch.float64) + torch.tril(_prune64(x, thr, temp, k["pruning_method"]), -1)) @ s
        (torch.clamp(p, 0.0, 1.0) * torch.tensor(w64[g])).sum().backward()
        pre[g] = p.detach().numpy()
        grad_iou[np.ix_(order[g], order[g])] = x.grad.numpy()
        grad_scores[order[g]] = s.grad.numpy()
    r2 = np.clip(pre, 0.0, 1.0)
    return dict(prob=r2, grad_scores=grad_scores, grad_iou=grad_iou, pre=pre, r2=r2, order=order, groups=groups, thresholded=False, vthr=vthr,
                mode="unmasked")


def test_unmasked_by_blocks_is_f64_layer():
    from oracle import oracle as O
    from groomed_nms_amd import synthetic
    from test_grad_iou_host import f64_layer
    rng = np.random.default_rng(77)
    boxes = synthetic.clustered_boxes_2d(rng, 500, 8)
    scores = synthetic.tie_free_scores(rng, 500)
    w = rng.uniform(-1, 2, size=500).astype(np.float32)
    m = O.iou2d(boxes, boxes)
    for kw in (dict(mask_group_boxes=False), dict(mask_group_boxes=False, pruning_method="sigmoidal", temperature=0.1, group_size=6)):
        a, b = f64_layer(O, scores, m, w, **kw), f64_unmasked_by_blocks(O, scores, m, w, **kw)
        assert np.array_equal(a["order"], b["order"]) and len(a["groups"]) == len(b["groups"])
        assert all(np.array_equal(x, y) for x, y in zip(a["groups"], b["groups"]))
        for key in ("prob", "pre", "r2", "grad_scores", "grad_iou"):
            np.testing.assert_allclose(b[key], a[key], rtol=1e-12, atol=1e-14, err_msg=key)
        assert np.array_equal(a["grad_iou"] != 0, b["grad_iou"] != 0)


def test_cotangent_layout_of_a_rectangular_matrix():
    """what overlaps hands gnms_iou2d_backward for a cotangent [B, M, N]: the row stride of the tensor it passes, never the row count"""
    from groomed_nms_amd.overlaps import _cotangent_layout
    for shape in [(2, 300, 257), (1, 1000, 5), (2, 5, 7), (1, 1, 1), (3, 1, 9), (1, 7, 1), (0, 4, 4), (2, 0, 4), (2, 4, 0)]:
        t, ld = _cotangent_layout(torch.zeros(shape), *shape)
        assert t.is_contiguous() and ld == max(shape[2], 1), shape
    wide = torch.zeros(2, 300, 300)[:, :, :257]                       # a slice of a wider buffer is used where it lies
    t, ld = _cotangent_layout(wide, 2, 300, 257)
    assert ld == 300 and t.data_ptr() == wide.data_ptr()
    for view in (torch.zeros(2, 257, 300).transpose(1, 2), torch.zeros(1, 1, 1).expand(2, 300, 257), torch.zeros(4, 300, 257)[::2],
                 torch.zeros(2, 300, 514)[:, :, ::2]):
        t, ld = _cotangent_layout(view, 2, 300, 257)
        assert t.is_contiguous() and ld == 257 and tuple(t.shape) == (2, 300, 257)


def test_header_and_ctypes_declare_the_new_entries():
    from groomed_nms_amd import _lib
    text = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gnms_iou2d_backward", "gnms_iou2d_backward_workspace_bytes", "gnms_backward_boxes", "gnms_backward_boxes_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in the header" % name
        assert name in _lib.EXPORTED_SYMBOLS, "%s has no ctypes signature" % name
    assert "GNMS_ABI_VERSION 1" in re.sub(r"\s+", " ", text)


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import build, _lib
    build.build()
    return _lib.load()


def _host(n):
    return (ctypes.c_float * max(n, 4))()


def test_iou2d_backward_argument_checks_run_before_any_launch(lib):
    """host pointers throughout: every call must fail in the checks (or be an empty problem), never reach a launch"""
    a, b, g, da, db = _host(64), _host(64), _host(256), _host(64), _host(64)
    ws = _host(4096)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)                     # noqa: E731
    call = lambda *args: lib.gnms_iou2d_backward(*args)               # noqa: E731
    assert call(p(a), p(b), p(g), -1, 4, 4, 4, p(da), p(db), p(ws), 16384, None) == -1 and b"negative" in lib.gnms_last_error()
    assert call(p(a), p(b), p(g), 1, -4, 4, 4, p(da), p(db), p(ws), 16384, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, -4, 4, p(da), p(db), p(ws), 16384, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, 4, 3, p(da), p(db), p(ws), 16384, None) == -1 and b"ld" in lib.gnms_last_error()
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, None, None, p(ws), 16384, None) == -1 and b"both outputs" in lib.gnms_last_error()
    assert call(p(a), None, p(g), 1, 4, 5, 5, p(da), None, p(ws), 16384, None) == -1          # boxes_b NULL needs M == N
    assert call(p(a), None, p(g), 1, 4, 4, 4, p(da), p(db), p(ws), 16384, None) == -1         # ... and d_boxes_b NULL
    assert call(None, p(b), p(g), 1, 4, 4, 4, p(da), p(db), p(ws), 16384, None) == -1
    assert call(p(a), p(b), None, 1, 4, 4, 4, p(da), p(db), p(ws), 16384, None) == -1
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, p(da), p(db), None, 16384, None) == -1
    need = lib.gnms_iou2d_backward_workspace_bytes(1, 4, 4)
    assert need > 0 and need % 256 == 0 and lib.gnms_iou2d_backward_workspace_bytes(0, 4, 4) == 0
    assert call(p(a), p(b), p(g), 1, 4, 4, 4, p(da), p(db), ctypes.c_void_p(256 * 1024), need - 1, None) == -4   # GNMS_ERR_WORKSPACE
    assert call(p(a), p(b), p(g), 0, 4, 4, 4, p(da), p(db), None, 0, None) == 0               # an empty batch is a success
    # the slabs are a fraction of the matrix: a unit is at least 32 rows x 256 columns, and leaves 16 bytes per row and per column,
    # so at most 16 / (256 * 4) + 16 / (32 * 4) of the matrix's bytes
    matrix = 8 * 4096 * 4096 * 4
    assert lib.gnms_iou2d_backward_workspace_bytes(8, 4096, 4096) <= matrix // 64 + matrix // 8 + 512


def test_backward_boxes_argument_checks_run_before_any_launch(lib):
    from groomed_nms_amd._lib import GnmsParams
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    gp, bx, sc, gs, gb = _host(8), _host(32), _host(8), _host(8), _host(32)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)                     # noqa: E731
    big = 1 << 30
    fake_ws = ctypes.c_void_p(256 * 4096)
    call = lambda *args: lib.gnms_backward_boxes(*args)               # noqa: E731
    assert call(p(gp), p(bx), p(sc), -1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(bx), p(sc), 1, -8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 7, 0, None, 0, fake_ws, big, None) == -1   # ld < N
    assert b"ld" in lib.gnms_last_error()
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), None, None, None, 8, 0, None, 0, fake_ws, big, None) == -1     # both outputs NULL
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), None, None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 7, None, 0, fake_ws, big, None) == -1   # unknown route
    assert call(p(gp), p(bx), p(sc), 1, 8, None, None, p(gs), p(gb), None, 8, 0, None, 0, fake_ws, big, None) == -1
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, None, big, None) == -1      # workspace NULL
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, fake_ws, 16, None) == -4    # ... too small
    # the dense route asks for its scratch before anything runs
    assert lib.gnms_backward_boxes_scratch_bytes(1, 8, 8, ctypes.byref(P), 0, 0) == 0           # default mode: the sparse route, no scratch
    need = lib.gnms_backward_boxes_scratch_bytes(1, 8, 8, ctypes.byref(P), 0, 1)
    assert need >= 2 * 8 * 8 * 4 and need > lib.gnms_backward_boxes_scratch_bytes(1, 8, 8, ctypes.byref(P), 1, 1) > 0
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 1, None, 0, fake_ws, big, None) == -1   # scratch NULL
    assert call(p(gp), p(bx), p(sc), 1, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 1, fake_ws, need - 1, fake_ws, big, None) == -4
    assert call(p(gp), p(bx), p(sc), 0, 8, None, ctypes.byref(P), p(gs), p(gb), None, 8, 0, None, 0, None, 0, None) == 0         # an empty batch
