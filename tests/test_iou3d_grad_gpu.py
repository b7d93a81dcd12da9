"""dL/dparams3d on the GPU: gnms_iou3d_backward against the float64 closed form of tests/test_iou3d_grad_host.py, its
Python face (overlaps.iou3d_batched(from_params=True) with a grad_fn), and the layer's cuboid gradient -- the one-call entry
differentiable_nms_with_iou3d_batched on both routes and the two-call composition -- against test_grad_iou_host.f64_layer's matrix
gradient contracted by that closed form.

Every comparison is held to the derived bound of test_iou3d_grad_host.py, chain_abs((n_i + 72) 2^-24 sum_j |g_ij| S_ij), plus -- where
the cotangent is itself only known to the suite's grad_iou tolerance (every mode but masked-linear, as in the 2D tests) --
sum_j (5e-4 + 1e-3 |g_ij|) |d overlap_ij|.  Stage 2 of the closed form is evaluated on the float32 extents the device saw (the min /
max of gnms_corners_of_cuboid's corners: the forward's own corners_of).  An element with no contributing term must be exactly 0.
Each case prints its largest error / bound ratio.
"""
import functools

import numpy as np
import pytest
import torch

from test_grad_iou_host import DEFAULTS, f64_layer, left_out
from test_iou_grad_host import bound_ratio, f64_unmasked_by_blocks
from test_iou3d_grad_host import (closed_form3d, closed_form3d_self, clustered_pair3d, cotangent3d, extents_of_corners, layer_reference3d,
                                  tie_cuboids)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import groomed_nms_amd as g
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return g


def dev(x):
    return torch.tensor(np.asarray(x), device="cuda")


def device_extents(params):
    """params [..., 7] ndarray -> [..., 6] float64: the extents of the corners the device computes (the forward's floats)"""
    from groomed_nms_amd import overlaps
    p = np.asarray(params, np.float32)
    flat = p.reshape(1, -1, 7)
    if flat.shape[1] == 0:
        return np.zeros(p.shape[:-1] + (6,))
    c = overlaps.corners_batched(dev(flat))[0].cpu().numpy()
    return extents_of_corners(c).reshape(p.shape[:-1] + (6,))


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. gnms_iou3d_backward
# ----------------------------------------------------------------------------------------------------------------------------------
def entry3(a, b, g, method=2, ld=None, want_a=True, want_b=True):
    """a [B, M, 7], b [B, N, 7] or None, g [B, M, N] ndarrays -> (d_a, d_b) ndarrays (None where not asked for), through the C entry"""
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B, M, _ = a.shape
    N = M if b is None else b.shape[1]
    ld = N if ld is None else ld
    gt = torch.full((B, M, max(ld, 1)), float("nan"), device="cuda")   # the padding columns must never be read into a result
    gt[:, :, :N] = dev(g)
    at, bt = dev(a), (None if b is None else dev(b))
    d_a = torch.full((B, M, 7), float("nan"), device="cuda") if want_a else None
    d_b = torch.full((B, N, 7), float("nan"), device="cuda") if (want_b and b is not None) else None
    ws = torch.empty((max(lib.gnms_iou3d_backward_workspace_bytes(B, M, N), 256),), dtype=torch.uint8, device="cuda")
    check(lib.gnms_iou3d_backward(ptr(at), ptr(bt), ptr(gt), B, M, N, ld, method, ptr(d_a), ptr(d_b), ptr(ws), ws.numel(), stream_ptr()),
          "gnms_iou3d_backward")
    torch.cuda.synchronize()
    return (None if d_a is None else d_a.cpu().numpy()), (None if d_b is None else d_b.cpu().numpy())


def rect_case(B, M, N, density=1.0, seed=0):
    if (M, N) == (1, 1):
        a = np.array([[[1.0, 1.5, 20.0, 1.6, 1.5, 4.0, 0.3]]] * B, np.float32)
        b = np.array([[[1.5, 1.3, 20.5, 1.7, 1.6, 3.8, -0.2]]] * B, np.float32)
    else:
        ab = [clustered_pair3d(17000 + seed + 13 * i + M + N, M, N) for i in range(B)]
        a, b = np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])
    g = np.stack([cotangent3d(seed + 5 * i + M * 3 + N, M, N, density) for i in range(B)])
    return a, b, g


def check_rect(tag, a, b, g, d_a, d_b, method=2):
    worst = 0.0
    ea, eb = device_extents(a), device_extents(b)
    for i in range(len(a)):
        f = closed_form3d(a[i], b[i], g[i], method, ea[i], eb[i])
        if d_a is not None:
            worst = max(worst, bound_ratio(d_a[i], f["d_a"], f["bound_a"]))
        if d_b is not None:
            worst = max(worst, bound_ratio(d_b[i], f["d_b"], f["bound_b"]))
    print("iou3d_backward %-36s error / bound %.3f" % (tag, worst))
    assert worst <= 1.0, tag


SHAPES = [(1, 1, 1, 2), (2, 5, 7, 2), (1, 64, 65, 2), (1, 257, 300, 2), (2, 500, 500, 2), (2, 5, 7, 0), (2, 5, 7, 1), (1, 257, 300, 0),
          (1, 257, 300, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d-method%d" % s for s in SHAPES])
def test_iou3d_backward_against_the_closed_form(G, shape):
    B, M, N, method = shape
    a, b, g = rect_case(B, M, N)
    d_a, d_b = entry3(a, b, g, method)
    assert np.isfinite(d_a).all() and np.isfinite(d_b).all()
    check_rect("dense %s" % (shape,), a, b, g, d_a, d_b, method)
    again = entry3(a, b, g, method)
    assert d_a.tobytes() == again[0].tobytes() and d_b.tobytes() == again[1].tobytes(), "two runs differ in their bits"


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 257, 300)], ids=["2x5x7", "1x257x300"])
def test_iou3d_backward_variants(G, shape):
    a, b, g = rect_case(*shape, seed=3)
    full = entry3(a, b, g)
    wide = entry3(a, b, g, ld=shape[2] + 5)                           # ld > N, not a multiple of 4
    assert full[0].tobytes() == wide[0].tobytes() and full[1].tobytes() == wide[1].tobytes()
    only_a = entry3(a, b, g, want_b=False)
    only_b = entry3(a, b, g, want_a=False)
    assert only_a[1] is None and only_b[0] is None
    assert only_a[0].tobytes() == full[0].tobytes() and only_b[1].tobytes() == full[1].tobytes()
    a, b, g = rect_case(*shape, density=0.01, seed=4)                 # 1 %-dense: most wave steps skip
    d_a, d_b = entry3(a, b, g)
    check_rect("1%% dense %s" % (shape,), a, b, g, d_a, d_b)


@pytest.mark.parametrize("n", [1, 65, 300, 500])
def test_iou3d_backward_self(G, n):
    """params_b = NULL: both roles summed into d_params_a"""
    B = 2 if n == 500 else 1
    x = np.stack([clustered_pair3d(17100 + n + i, n, 1)[0] for i in range(B)])
    g = np.stack([cotangent3d(n + i, n, n) for i in range(B)])
    d, none = entry3(x, None, g)
    assert none is None
    e = device_extents(x)
    worst = 0.0
    for i in range(B):
        f = closed_form3d_self(x[i], g[i], 2, e[i])
        worst = max(worst, bound_ratio(d[i], f["d"], f["bound"]))
    print("iou3d_backward self n=%-4d error / bound %.3f" % (n, worst))
    assert worst <= 1.0
    assert d.tobytes() == entry3(x, None, g)[0].tobytes()


@pytest.mark.parametrize("k", [1, 13])
def test_iou3d_backward_ties(G, k):
    """touching in y (1/2), touching in x (1), identical boxes, ry = 0 (d ry is the symmetric value, exactly 0), shared edges; the flat
    pairs (degenerate hull, zero volume) have all-zero cotangents: their rows are exactly 0 and nothing is NaN"""
    a, b = tie_cuboids(50 + k, k)
    kind = np.arange(len(a)) % 6
    g = cotangent3d(k, len(a), len(b))
    g[kind == 5, :] = 0.0
    g[:, kind == 5] = 0.0
    assert np.array_equal(device_extents(a), device_extents(a).astype(np.float32))
    for method in (0, 1, 2):
        d_a, d_b = entry3(a[None], b[None], g[None], method)
        assert np.isfinite(d_a).all() and np.isfinite(d_b).all(), "a zero cotangent let a NaN through"
        assert not d_a[0][kind == 5].any() and not d_b[0][kind == 5].any()
        assert not d_a[0][:, 6].any() and not d_b[0][:, 6].any(), "ry = 0: d ry is the symmetric value"
        check_rect("ties %d x %d method %d" % (len(a), len(b), method), a[None], b[None], g[None], d_a, d_b, method)
    gs = cotangent3d(k + 1, len(a), len(a))
    gs[kind == 5, :] = 0.0
    gs[:, kind == 5] = 0.0
    d, _ = entry3(a[None], None, gs[None])
    f = closed_form3d_self(a, gs, 2, device_extents(a))
    assert np.isfinite(d).all() and bound_ratio(d[0], f["d"], f["bound"]) <= 1.0
    # identical boxes, one pair at a time: the closed form is exactly 0 in each role, the device within its bound of that
    sel = np.zeros((len(a), len(b)), np.float32)
    sel[kind == 0, kind == 0] = 1.5
    d_a, d_b = entry3(a[None], b[None], sel[None])
    f = closed_form3d(a, b, sel, 2, device_extents(a), device_extents(b))
    assert not f["d_a"].any() and not f["d_b"].any()
    assert bound_ratio(d_a[0], f["d_a"], f["bound_a"]) <= 1.0 and bound_ratio(d_b[0], f["d_b"], f["bound_b"]) <= 1.0


def test_iou3d_backward_exact_zeros(G):
    # an all-zero cotangent over zero-extent cuboids: 0, not 0 * NaN
    a = np.zeros((1, 70, 7), np.float32)
    a[0, :, 0] = np.arange(70)
    b = a[:, :66].copy()
    for method in (0, 1, 2):
        d_a, d_b = entry3(a, b, np.zeros((1, 70, 66), np.float32), method)
        assert d_a.tobytes() == np.zeros_like(d_a).tobytes() and d_b.tobytes() == np.zeros_like(d_b).tobytes()
    d, _ = entry3(a, None, np.zeros((1, 70, 70), np.float32))
    assert d.tobytes() == np.zeros_like(d).tobytes()
    # one zero-extent box among sane ones, its row and column of the cotangent 0: its gradient is exactly 0, nothing is NaN
    a, b, g = rect_case(1, 70, 66, seed=9)
    a[0, 11, 3:6] = 0.0
    g[0, 11, :] = 0.0
    d_a, d_b = entry3(a, b, g)
    assert np.isfinite(d_a).all() and np.isfinite(d_b).all() and not d_a[0, 11].any()


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. overlaps.iou3d_batched(from_params=True)
# ----------------------------------------------------------------------------------------------------------------------------------
def test_iou3d_batched_backward_is_the_entry(G):
    from groomed_nms_amd import overlaps
    a, b, g = rect_case(2, 257, 300, seed=21)
    for method, kw in ((1, dict(method="generalized")), (0, dict(method="normal")), (2, dict(nms_overlap=True))):
        want = entry3(a, b, g, method)
        ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        out = overlaps.iou3d_batched(ta, tb, from_params=True, **kw)
        assert out.grad_fn is not None
        assert torch.equal(out.detach(), overlaps.iou3d_batched(ta.detach(), tb.detach(), from_params=True, **kw))
        out.backward(dev(g))
        assert ta.grad.cpu().numpy().tobytes() == want[0].tobytes() and tb.grad.cpu().numpy().tobytes() == want[1].tobytes()
    # one side only
    ta2 = dev(a).requires_grad_(True)
    overlaps.iou3d_batched(ta2, dev(b), from_params=True, nms_overlap=True).backward(dev(g))
    assert torch.equal(ta2.grad, ta.grad)
    # the one-set form (b is a, b = None), with and without the threshold, under a transposed cotangent too
    x, gs = a[:, :200], np.ascontiguousarray(g[:, :200, :200])
    want = entry3(x, None, gs)[0]
    for kw in (dict(), dict(nms_threshold=0.4)):
        for same in (False, True):
            for cot in (dev(gs), dev(gs).transpose(1, 2).contiguous().transpose(1, 2)):
                tx = dev(x).requires_grad_(True)
                out = overlaps.iou3d_batched(tx, tx if same else None, from_params=True, nms_overlap=True, **kw)
                assert out.grad_fn is not None
                out.backward(cot)
                assert tx.grad.cpu().numpy().tobytes() == want.tobytes()
    # a transposed cotangent of the rectangular form
    ta3, tb3 = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    overlaps.iou3d_batched(ta3, tb3, from_params=True, nms_overlap=True).backward(dev(g).transpose(1, 2).contiguous().transpose(1, 2))
    assert torch.equal(ta3.grad, ta.grad) and torch.equal(tb3.grad, tb.grad)
    # `out` with a gradient, other dtypes
    with pytest.raises(ValueError):
        overlaps.iou3d_batched(dev(a).requires_grad_(True), dev(b), from_params=True, out=torch.empty((2, 257, 300), device="cuda"))
    with pytest.raises(TypeError):
        overlaps.iou3d_batched(dev(a).double().requires_grad_(True), dev(b).double(), from_params=True)
    # inputs without grad yield a leaf whose bytes are today's call
    leaf = overlaps.iou3d_batched(dev(a), dev(b), from_params=True, nms_overlap=True)
    assert leaf.grad_fn is None and not leaf.requires_grad
    with torch.no_grad():
        quiet = overlaps.iou3d_batched(ta, tb, from_params=True, nms_overlap=True)
    assert quiet.grad_fn is None and torch.equal(quiet, leaf)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. the layer
# ----------------------------------------------------------------------------------------------------------------------------------
MODE_KW = {
    "default": dict(),
    "cap5": dict(group_size=5),
    "unmasked": dict(mask_group_boxes=False),
    "ungrouped": dict(group_boxes=False),
    "sigmoidal": dict(pruning_method="sigmoidal", temperature=0.1),
}
PER = {"default": 32, "cap5": 32, "unmasked": 8, "ungrouped": 8, "sigmoidal": 32}
# one wave, the reference's size, beyond the one-launch limit; the default mode also beyond 4096 (the matrix write takes the side stream)
LAYER_CASES = [(n, mode) for mode in MODE_KW for n in (37, 500, 1100)] + [(4160, "default")]
SPARSE_MODES = ("default", "cap5", "sigmoidal")                       # masked groups: AUTO takes the sparse route


# A box whose rescored probability sits within the margin of a clamp bound reaches EVERY gradient of the ungrouped mode (reference_of
# refuses such an input): that case takes the next seed of its sequence.  A condition on the inputs, as the fixture's maker has them.
SEED_SHIFT = {(1100, "ungrouped", 0): 1}


def layer_inputs(n, mode, image=0):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(18000 + 17 * n + 3 * sorted(MODE_KW).index(mode) + 101 * image + 1009 * SEED_SHIFT.get((n, mode, image), 0))
    params = synthetic.boxes_3d(rng, n, clustered=True, per=min(PER[mode], n))
    scores = synthetic.tie_free_scores(rng, n)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    return params, scores, w


def device_overlap(params, thr):
    """the forward's own float32 matrix of one image (the grouping decisions of the float64 layer are taken on it)"""
    from groomed_nms_amd import overlaps
    return overlaps.iou3d_batched(dev(params[None]), from_params=True, nms_overlap=True, nms_threshold=thr)[0].cpu().numpy()


def reference_of(params, scores, w, mode):
    """dict(ref [n, 7], bound, skip (bool over input indices: boxes a near-tie decision reaches), heads (bool)) from the float64 layer"""
    from oracle import oracle as O
    kw = MODE_KW[mode]
    n = len(scores)
    if n == 0:
        return dict(ref=np.zeros((0, 7)), bound=np.zeros((0, 7)), skip=np.zeros(0, bool), heads=np.zeros(0, bool))
    k = dict(DEFAULTS)
    k.update(kw)
    m = device_overlap(params, k["nms_threshold"])
    f = f64_unmasked_by_blocks(O, scores, m, w, **kw) if (mode == "unmasked" and n > 1100) else f64_layer(O, scores, m, w, **kw)
    n_und, skip = left_out(f)
    assert n_und <= max(1, n // 100), "%d of %d boxes sit within the margin of a clamp bound or the threshold" % (n_und, n)
    assert n_und == 0 or f["mode"] != "ungrouped", "an undecided box reaches every gradient of the ungrouped mode"
    masked_linear = k["group_boxes"] and k["mask_group_boxes"] and k["pruning_method"] == "linear"
    ext = device_extents(params)
    ref, bound = layer_reference3d(params, f["grad_iou"], ext=ext, cot_tol=not masked_linear)
    heads = np.zeros(n, bool)
    for g in f["groups"]:
        heads[f["order"][g[0]]] = True
    return dict(ref=ref, bound=bound, skip=skip, heads=heads, prob=f["prob"], ext=ext)


@functools.lru_cache(maxsize=None)
def layer_case(n, mode):
    params, scores, w = layer_inputs(n, mode)
    r = reference_of(params, scores, w, mode)
    for a in (params, scores, w):
        a.setflags(write=False)
    return params, scores, w, r


def run_entry(G, entry, params, scores, w, kw, box_grad=True, counts=None, keep_matrix_grad=False):
    """params [B, n, 7], scores / w [B, n] ndarrays -> (prob, grad_scores, grad_params or None[, matrix gradient]) device tensors"""
    from groomed_nms_amd import overlaps
    pt = dev(params).requires_grad_(box_grad)
    st = dev(scores).requires_grad_(True)
    wt = dev(w)
    ct = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    m = None
    if entry == "with_iou3d":
        out = G.differentiable_nms_with_iou3d_batched(st, pt, counts=ct, **kw)
        prob = out[0]
        assert out[6].grad_fn is None and not out[6].requires_grad, "the returned matrix stays non-differentiable"
    else:
        assert counts is None
        k = dict(DEFAULTS)
        k.update(kw)
        m = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True, nms_threshold=k["nms_threshold"])
        if keep_matrix_grad:
            m.retain_grad()
        prob = G.differentiable_nms_batched(st, m, **kw)[0]
    (prob * wt).sum().backward()
    if keep_matrix_grad:
        return prob.detach(), st.grad, pt.grad, m.grad
    return prob.detach(), st.grad, pt.grad


def check_layer(tag, got, r):
    keep = ~r["skip"]
    ratio = bound_ratio(got[keep], r["ref"][keep], r["bound"][keep])
    print("layer3d %-44s error / bound %.3f  (largest |grad| %.3e, %d boxes left out)" % (tag, ratio, float(np.abs(r["ref"]).max()), int(r["skip"].sum())))
    assert ratio <= 1.0, tag


@pytest.mark.parametrize("n,mode", LAYER_CASES, ids=["%d-%s" % c for c in LAYER_CASES])
def test_layer_cuboid_gradient(G, n, mode):
    from groomed_nms_amd import groomed_nms as GN
    params, scores, w, r = layer_case(n, mode)
    kw = MODE_KW[mode]
    prob, gs, gp = run_entry(G, "with_iou3d", params[None], scores[None], w[None], kw)
    assert gp is not None, "params3d.grad is None"
    assert tuple(gp.shape) == (1, n, 7) and bool(torch.isfinite(gp).all())
    auto = gp[0].cpu().numpy()
    check_layer("with_iou3d n=%d %s" % (n, mode), auto, r)
    # prob and dL/dscores are the bits of the call without the cuboid gradient
    prob0, gs0, none = run_entry(G, "with_iou3d", params[None], scores[None], w[None], kw, box_grad=False)
    assert none is None
    assert torch.equal(prob, prob0), "prob changed"
    assert torch.equal(gs, gs0), "grad_scores changed"
    np.testing.assert_allclose(prob[0].cpu().numpy(), r["prob"], atol=1e-4, rtol=0)
    # the same inputs give the same bits
    assert torch.equal(gp, run_entry(G, "with_iou3d", params[None], scores[None], w[None], kw)[2])
    # the dense route: within the bound everywhere; a non-head member has one term there as on the sparse route -- the same bits
    assert GN.BOX_GRAD_ROUTE == "auto"
    GN.BOX_GRAD_ROUTE = "dense"
    try:
        probd, gsd, gpd = run_entry(G, "with_iou3d", params[None], scores[None], w[None], kw)
    finally:
        GN.BOX_GRAD_ROUTE = "auto"
    dense = gpd[0].cpu().numpy()
    check_layer("dense route n=%d %s" % (n, mode), dense, r)
    assert torch.equal(probd, prob0) and torch.equal(gsd, gs0)
    if mode in SPARSE_MODES:
        members = ~r["heads"]
        assert members.sum() > 0 and r["heads"].sum() > 0
        assert np.array_equal(auto[members], dense[members]), "a member's gradient has one term: the two routes must give the same bits"
        assert auto[members].any()
    else:
        assert auto.tobytes() == dense.tobytes()                      # AUTO is the dense route in these modes
    # the two-call composition reaches params3d.grad through grad_iou: the same figure
    prob2, gs2, gp2 = run_entry(G, "two_call", params[None], scores[None], w[None], kw)
    check_layer("two_call n=%d %s" % (n, mode), gp2[0].cpu().numpy(), r)
    assert torch.equal(prob2, prob0)


@pytest.mark.parametrize("n,mode", LAYER_CASES, ids=["%d-%s" % c for c in LAYER_CASES])
def test_cuboid_gradient_against_its_own_cotangent(G, n, mode):
    """The bound of test_layer_cuboid_gradient carries, outside masked-linear, the tolerance of the matrix gradient, which dwarfs the
    cuboid-gradient arithmetic's own error there.  This holds that arithmetic alone, in every mode: params3d.grad against the float64
    closed form contracted with the float32 matrix gradient the layer ACTUALLY produced (retained on the way), to the bound without
    that term; and the one-call entry's dense route against the same figure."""
    from groomed_nms_amd import groomed_nms as GN
    params, scores, w, r = layer_case(n, mode)
    kw = MODE_KW[mode]
    _, _, gp, gm = run_entry(G, "two_call", params[None], scores[None], w[None], kw, keep_matrix_grad=True)
    g = gm[0].cpu().numpy()
    assert g.any()
    f = closed_form3d_self(params, g, 2, r["ext"])
    ratio = bound_ratio(gp[0].cpu().numpy(), f["d"], f["bound"])
    GN.BOX_GRAD_ROUTE = "dense"
    try:
        dense = run_entry(G, "with_iou3d", params[None], scores[None], w[None], kw)[2][0].cpu().numpy()
    finally:
        GN.BOX_GRAD_ROUTE = "auto"
    ratio_d = bound_ratio(dense, f["d"], f["bound"])
    print("layer3d n=%d %-10s against its own cotangent: error / bound two_call %.3f, dense route %.3f (%d non-zero cotangents)"
          % (n, mode, ratio, ratio_d, int((g != 0).sum())))
    assert ratio <= 1.0 and ratio_d <= 1.0


@pytest.mark.parametrize("mode", ["default", "unmasked"])
@pytest.mark.parametrize("n", [37, 500])
def test_ragged_counts_with_an_empty_image(G, n, mode):
    counts = [n, 0, n - n // 3]
    params = np.zeros((3, n, 7), np.float32)
    scores = np.zeros((3, n), np.float32)
    w = np.zeros((3, n), np.float32)
    refs = []
    for b, c in enumerate(counts):
        px, sc, ww = layer_inputs(n, mode, image=b + 1)
        params[b], scores[b], w[b] = px, sc, ww
        refs.append(reference_of(px[:c], sc[:c], ww[:c], mode))
    prob, gs, gp = run_entry(G, "with_iou3d", params, scores, w, MODE_KW[mode], counts=counts)
    gp = gp.cpu().numpy()
    for b, c in enumerate(counts):
        assert not gp[b, c:].any(), "boxes behind counts[b] get exactly 0"
        if c:
            check_layer("with_iou3d n=%d %s image %d (%d boxes)" % (n, mode, b, c), gp[b, :c], refs[b])
    prob0, gs0, _ = run_entry(G, "with_iou3d", params, scores, w, MODE_KW[mode], box_grad=False, counts=counts)
    assert torch.equal(prob, prob0) and torch.equal(gs, gs0)


def test_forward_and_backward_in_a_graph(G):
    """captured once, replayed on other contents: the replay's bits are eager's (B = 2, N = 500, default mode)"""
    n, mode = 500, "default"
    kw = MODE_KW[mode]

    def batch(i):
        cases = [layer_inputs(n, mode, image=i), layer_inputs(n, mode, image=i + 1)]
        return tuple(np.stack([c[k] for c in cases]) for k in range(3))
    cases = [batch(7), batch(9)]
    eager = [run_entry(G, "with_iou3d", p, s, w, kw) for p, s, w in cases]
    pt = dev(cases[0][0]).requires_grad_(True)
    st = dev(cases[0][1]).requires_grad_(True)
    wt = dev(cases[0][2])

    def step():
        prob = G.differentiable_nms_with_iou3d_batched(st, pt, **kw)[0]
        return (prob,) + torch.autograd.grad((prob * wt).sum(), (st, pt))
    step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = step()
    torch.cuda.synchronize()
    for which in (1, 0):
        with torch.no_grad():
            pt.copy_(dev(cases[which][0]))
            st.copy_(dev(cases[which][1]))
            wt.copy_(dev(cases[which][2]))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[which]):
            assert torch.equal(got.detach(), want), "the replay differs from the eager run"
