"""dL/dboxes on the GPU: gnms_iou2d_backward against the float64 closed form of tests/test_iou_grad_host.py, its Python
face (overlaps.iou_batched / iou with a grad_fn), and the layer's box gradient -- the two one-call entries and the two-call
composition differentiable_nms(scores, iou(boxes, boxes)) -- against test_grad_iou_host.f64_layer's matrix gradient contracted by
that closed form.

Every comparison is held to the derived bound of test_iou_grad_host.py, (n_i + 16) 2^-24 sum_j |g_ij| S_ijk, plus -- where the
cotangent is itself only known to the suite's grad_iou tolerance (every mode but masked-linear) -- sum_j (5e-4 + 1e-3 |g_ij|) |dIoU_ij|.
An element with no contributing term must be exactly 0.  Each case prints its largest error / bound ratio.
"""
import functools

import numpy as np
import pytest
import torch

from test_grad_iou_host import DEFAULTS, f64_layer, left_out
from test_iou_grad_host import (bound_ratio, closed_form, closed_form_self, clustered_pair, cotangent, f64_unmasked_by_blocks,
                                layer_reference, tie_boxes)

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


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. gnms_iou2d_backward
# ----------------------------------------------------------------------------------------------------------------------------------
def entry2(a, b, g, ld=None, want_a=True, want_b=True):
    """a [B, M, 4], b [B, N, 4] or None, g [B, M, N] ndarrays -> (d_a, d_b) ndarrays (None where not asked for), through the C entry"""
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    B, M, _ = a.shape
    N = M if b is None else b.shape[1]
    ld = N if ld is None else ld
    gt = torch.full((B, M, max(ld, 1)), float("nan"), device="cuda")   # the padding columns must never be read into a result
    gt[:, :, :N] = dev(g)
    at, bt = dev(a), (None if b is None else dev(b))
    d_a = torch.full((B, M, 4), float("nan"), device="cuda") if want_a else None
    d_b = torch.full((B, N, 4), float("nan"), device="cuda") if (want_b and b is not None) else None
    ws = torch.empty((max(lib.gnms_iou2d_backward_workspace_bytes(B, M, N), 256),), dtype=torch.uint8, device="cuda")
    check(lib.gnms_iou2d_backward(ptr(at), ptr(bt), ptr(gt), B, M, N, ld, ptr(d_a), ptr(d_b), ptr(ws), ws.numel(), stream_ptr()),
          "gnms_iou2d_backward")
    torch.cuda.synchronize()
    return (None if d_a is None else d_a.cpu().numpy()), (None if d_b is None else d_b.cpu().numpy())


def rect_case(B, M, N, density=1.0, seed=0):
    ab = [clustered_pair(7000 + seed + 13 * i + M + N, M, N) for i in range(B)]
    a, b = np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])
    g = np.stack([cotangent(seed + 5 * i + M * 3 + N, M, N, density) for i in range(B)])
    return a, b, g


def check_rect(tag, a, b, g, d_a, d_b):
    worst = 0.0
    for i in range(len(a)):
        f = closed_form(a[i], b[i], g[i])
        if d_a is not None:
            worst = max(worst, bound_ratio(d_a[i], f["d_a"], f["bound_a"]))
        if d_b is not None:
            worst = max(worst, bound_ratio(d_b[i], f["d_b"], f["bound_b"]))
    print("iou2d_backward %-28s error / bound %.3f" % (tag, worst))
    assert worst <= 1.0, tag


SHAPES = [(1, 1, 1), (2, 5, 7), (1, 64, 65), (1, 257, 300), (2, 500, 500)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_iou2d_backward_against_the_closed_form(G, shape):
    a, b, g = rect_case(*shape)
    d_a, d_b = entry2(a, b, g)
    check_rect("dense %s" % (shape,), a, b, g, d_a, d_b)
    again = entry2(a, b, g)
    assert d_a.tobytes() == again[0].tobytes() and d_b.tobytes() == again[1].tobytes(), "two runs differ in their bits"


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 257, 300)], ids=["2x5x7", "1x257x300"])
def test_iou2d_backward_variants(G, shape):
    a, b, g = rect_case(*shape, seed=3)
    full = entry2(a, b, g)
    wide = entry2(a, b, g, ld=shape[2] + 5)                           # ld > N, not a multiple of 4
    assert full[0].tobytes() == wide[0].tobytes() and full[1].tobytes() == wide[1].tobytes()
    only_a = entry2(a, b, g, want_b=False)
    only_b = entry2(a, b, g, want_a=False)
    assert only_a[1] is None and only_b[0] is None
    assert only_a[0].tobytes() == full[0].tobytes() and only_b[1].tobytes() == full[1].tobytes()
    a, b, g = rect_case(*shape, density=0.01, seed=4)                 # 1 %-dense: most wave steps skip
    d_a, d_b = entry2(a, b, g)
    check_rect("1%% dense %s" % (shape,), a, b, g, d_a, d_b)


@pytest.mark.parametrize("n", [1, 65, 300, 500])
def test_iou2d_backward_self(G, n):
    """boxes_b = NULL: both roles summed into d_boxes_a"""
    B = 2 if n == 500 else 1
    x = np.stack([clustered_pair(7100 + n + i, n, 1)[0] for i in range(B)])
    g = np.stack([cotangent(n + i, n, n) for i in range(B)])
    d, none = entry2(x, None, g)
    assert none is None
    worst = 0.0
    for i in range(B):
        f = closed_form_self(x[i], g[i])
        worst = max(worst, bound_ratio(d[i], f["d"], f["bound"]))
    print("iou2d_backward self n=%-4d error / bound %.3f" % (n, worst))
    assert worst <= 1.0
    assert d.tobytes() == entry2(x, None, g)[0].tobytes()
    # the diagonal alone: a self pair's derivative is exactly 0
    gd = np.stack([np.diag(np.linspace(0.5, 2, n)).astype(np.float32)] * B)
    assert not entry2(x, None, gd)[0].any()


def test_iou2d_backward_exact_zeros(G):
    # an all-zero cotangent over degenerate (zero-area) boxes: 0, not 0 * NaN
    a = np.zeros((1, 70, 4), np.float32)
    a[0, :, 0] = a[0, :, 2] = np.arange(70)
    b = a[:, :66].copy()
    z = np.zeros((1, 70, 66), np.float32)
    d_a, d_b = entry2(a, b, z)
    assert d_a.tobytes() == np.zeros_like(d_a).tobytes() and d_b.tobytes() == np.zeros_like(d_b).tobytes()
    d, _ = entry2(a, None, np.zeros((1, 70, 70), np.float32))
    assert d.tobytes() == np.zeros_like(d).tobytes()
    # disjoint boxes under a dense cotangent: inter = 0 and no clamp passes (d < 0 on the x axis)
    a, b, g = rect_case(1, 70, 66, seed=9)
    a[..., [0, 2]] = (a[..., [0, 2]] % 100.0) + np.array([0.0, 120.0], np.float32)      # x in [0, 220)
    b[..., [0, 2]] = (b[..., [0, 2]] % 100.0) + np.array([1000.0, 1120.0], np.float32)  # x in [1000, 1220)
    d_a, d_b = entry2(a, b, g)
    assert not d_a.any() and not d_b.any()


@pytest.mark.parametrize("k", [1, 13, 60])
def test_iou2d_backward_ties(G, k):
    a, b = tie_boxes(50 + k, k)
    g = cotangent(k, len(a), len(b))
    d_a, d_b = entry2(a[None], b[None], g[None])
    check_rect("ties %d x %d" % (len(a), len(b)), a[None], b[None], g[None], d_a, d_b)
    d, _ = entry2(a[None], None, g[None])
    f = closed_form_self(a, g)
    assert bound_ratio(d[0], f["d"], f["bound"]) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. overlaps.iou_batched / overlaps.iou
# ----------------------------------------------------------------------------------------------------------------------------------
def test_iou_batched_backward_is_the_entry(G):
    from groomed_nms_amd import overlaps
    a, b, g = rect_case(2, 257, 300, seed=21)
    want = entry2(a, b, g)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    out = overlaps.iou_batched(ta, tb)
    assert out.grad_fn is not None and torch.equal(out.detach(), overlaps.iou_batched(ta.detach(), tb.detach()))
    out.backward(dev(g))
    assert ta.grad.cpu().numpy().tobytes() == want[0].tobytes() and tb.grad.cpu().numpy().tobytes() == want[1].tobytes()
    # one side only
    ta2 = dev(a).requires_grad_(True)
    overlaps.iou_batched(ta2, dev(b)).backward(dev(g))
    assert torch.equal(ta2.grad, ta.grad)
    # boxes on both sides
    x, gs = a[:, :200], g[:, :200, :200]
    tx = dev(x).requires_grad_(True)
    overlaps.iou_batched(tx).backward(dev(gs))
    assert tx.grad.cpu().numpy().tobytes() == entry2(x, None, gs)[0].tobytes()
    # inputs without grad yield a leaf, as before
    leaf = overlaps.iou_batched(dev(a), dev(b))
    assert leaf.grad_fn is None and not leaf.requires_grad
    with torch.no_grad():
        assert overlaps.iou_batched(ta, tb).grad_fn is None


RECT = [(2, 300, 257), (1, 1000, 5), (1, 5, 1000), (2, 257, 300), (3, 1, 9), (1, 70, 1)]


@pytest.mark.parametrize("form", ["contiguous", "transposed", "wide", "expanded", "batch_strided"])
@pytest.mark.parametrize("shape", RECT, ids=["%dx%dx%d" % s for s in RECT])
def test_iou_batched_backward_rectangular_and_strided_cotangents(G, shape, form):
    """more rows than columns, fewer, a single row or column; the cotangent as autograd may hand it over: contiguous, the transpose of a
    contiguous [B, N, M], a slice of a wider buffer (used where it lies, ld > N), a broadcast value, every other image of a larger
    batch.  Each equals the C entry on the same values bit for bit, and the entry is within the bound."""
    from groomed_nms_amd import overlaps
    B, M, N = shape
    a, b, g = rect_case(B, M, N, seed=31)
    if form == "expanded":
        g = np.broadcast_to(np.float32(0.75), (B, M, N)).copy()
    want = entry2(a, b, g)
    check_rect("%s %s" % (form, shape), a, b, g, want[0], want[1])
    gt = dev(g)
    if form == "transposed":
        cot = gt.transpose(1, 2).contiguous().transpose(1, 2)
        assert not cot.is_contiguous() or M == 1 or N == 1
    elif form == "wide":
        wide = torch.full((B, M, N + 7), float("nan"), device="cuda")
        wide[:, :, :N] = gt
        cot = wide[:, :, :N]
    elif form == "expanded":
        cot = torch.full((1, 1, 1), 0.75, device="cuda").expand(B, M, N)
    elif form == "batch_strided":
        big = torch.full((2 * B, M, N), float("nan"), device="cuda")
        big[::2] = gt
        cot = big[::2]
    else:
        cot = gt
    assert torch.equal(cot, gt)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    overlaps.iou_batched(ta, tb).backward(cot)
    assert ta.grad.cpu().numpy().tobytes() == want[0].tobytes() and tb.grad.cpu().numpy().tobytes() == want[1].tobytes()
    if B == 1:                                                        # the reference's own signature, 2-D in and out
        ua, ub = dev(a[0]).requires_grad_(True), dev(b[0]).requires_grad_(True)
        overlaps.iou(ua, ub).backward(cot[0])
        assert ua.grad.cpu().numpy().tobytes() == want[0][0].tobytes() and ub.grad.cpu().numpy().tobytes() == want[1][0].tobytes()


def test_iou_of_a_tensor_with_itself_takes_the_one_set_form(G):
    """iou(x, x) on ONE tensor: both roles summed by gnms_iou2d_backward itself (boxes_b = NULL), also under a transposed cotangent"""
    from groomed_nms_amd import overlaps
    n = 300
    x = clustered_pair(7300, n, 1)[0]
    g = cotangent(41, n, n)
    want = entry2(x[None], None, g[None])[0][0]
    f = closed_form_self(x, g)
    assert bound_ratio(want, f["d"], f["bound"]) <= 1.0
    for cot in (dev(g), dev(g).t().contiguous().t()):
        tx = dev(x).requires_grad_(True)
        overlaps.iou(tx, tx).backward(cot)
        assert tx.grad.cpu().numpy().tobytes() == want.tobytes()
    # two tensors with the same values take the two-set form: the same gradient to the bound, summed by autograd
    ta, tb = dev(x).requires_grad_(True), dev(x).requires_grad_(True)
    overlaps.iou(ta, tb).backward(dev(g))
    assert bound_ratio((ta.grad + tb.grad).cpu().numpy(), f["d"], f["bound"]) <= 1.0


def test_iou_backward_is_the_entry(G):
    from groomed_nms_amd import overlaps
    a, b, g = rect_case(1, 64, 65, seed=22)
    want = entry2(a, b, g)
    ta, tb = dev(a[0]).requires_grad_(True), dev(b[0]).requires_grad_(True)
    m = overlaps.iou(ta, tb)
    assert m.grad_fn is not None and tuple(m.shape) == (64, 65)
    m.backward(dev(g[0]))
    assert ta.grad.cpu().numpy().tobytes() == want[0][0].tobytes() and tb.grad.cpu().numpy().tobytes() == want[1][0].tobytes()
    leaf = overlaps.iou(dev(a[0]), dev(b[0]))
    assert leaf.grad_fn is None and not leaf.requires_grad
    # mode='list' is torch arithmetic and no longer detaches
    tl = dev(a[0]).requires_grad_(True)
    overlaps.iou(tl, dev(b[0][:64]), mode="list").sum().backward()
    i = np.arange(64)
    sel = np.zeros((64, 64), np.float32)
    sel[i, i] = 1.0
    f = closed_form(a[0], b[0][:64], sel)
    assert bound_ratio(tl.grad.cpu().numpy(), f["d_a"], f["bound_a"]) <= 1.0


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
# one wave, the reference's size, beyond the one-launch limit, beyond 4096 (the last two modes stop at 1100)
LAYER_CASES = [(n, mode) for mode in MODE_KW for n in (37, 500, 1100, 4160) if not (n == 4160 and mode in ("ungrouped", "sigmoidal"))]
ENTRIES = ("with_iou2d", "from_boxes", "two_call")
# (the from-boxes entry has the grouped modes only)
LAYER_PARAMS = [(n, mode, entry) for n, mode in LAYER_CASES for entry in ENTRIES if not (entry == "from_boxes" and mode == "ungrouped")]
SPARSE_PARAMS = [(n, mode) for n, mode in LAYER_CASES if mode in ("default", "cap5", "sigmoidal")]


def layer_inputs(n, mode, image=0):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(8000 + 17 * n + 3 * sorted(MODE_KW).index(mode) + 101 * image)
    boxes = synthetic.clustered_boxes_2d(rng, n, min(PER[mode], n))
    scores = synthetic.tie_free_scores(rng, n)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    return boxes, scores, w


def reference_of(boxes, scores, w, mode):
    """dict(ref [n, 4], bound, skip (bool over input indices: boxes a near-tie decision reaches), heads (bool)) from the float64 layer"""
    from oracle import oracle as O
    kw = MODE_KW[mode]
    n = len(scores)
    if n == 0:
        return dict(ref=np.zeros((0, 4)), bound=np.zeros((0, 4)), skip=np.zeros(0, bool), heads=np.zeros(0, bool))
    m = O.iou2d(boxes, boxes)
    # (unmasked groups beyond the reference's size: the same float64 layer group by group, pinned against f64_layer on the host)
    f = f64_unmasked_by_blocks(O, scores, m, w, **kw) if (mode == "unmasked" and n > 1100) else f64_layer(O, scores, m, w, **kw)
    n_und, skip = left_out(f)
    assert n_und <= max(1, n // 100), "%d of %d boxes sit within the margin of a clamp bound or the threshold" % (n_und, n)
    assert n_und == 0 or f["mode"] != "ungrouped", "an undecided box reaches every gradient of the ungrouped mode"
    k = dict(DEFAULTS)
    k.update(kw)
    masked_linear = k["group_boxes"] and k["mask_group_boxes"] and k["pruning_method"] == "linear"
    ref, bound = layer_reference(boxes, f["grad_iou"], cot_tol=not masked_linear)
    heads = np.zeros(n, bool)
    for g in f["groups"]:
        heads[f["order"][g[0]]] = True
    return dict(ref=ref, bound=bound, skip=skip, heads=heads, prob=f["prob"])


@functools.lru_cache(maxsize=None)
def layer_case(n, mode):
    boxes, scores, w = layer_inputs(n, mode)
    r = reference_of(boxes, scores, w, mode)
    for a in (boxes, scores, w):
        a.setflags(write=False)
    return boxes, scores, w, r


def run_entry(G, entry, boxes, scores, w, kw, box_grad=True, counts=None):
    """boxes [B, n, 4], scores / w [B, n] ndarrays -> (prob, grad_scores, grad_boxes or None) device tensors"""
    from groomed_nms_amd import overlaps
    bt = dev(boxes).requires_grad_(box_grad)
    st = dev(scores).requires_grad_(True)
    wt = dev(w)
    ct = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    if entry == "with_iou2d":
        out = G.differentiable_nms_with_iou2d_batched(st, bt, counts=ct, **kw)
        prob = out[0]
        assert out[6].grad_fn is None and not out[6].requires_grad, "the returned matrix stays non-differentiable"
    elif entry == "from_boxes":
        prob = G.differentiable_nms_from_boxes_batched(st, bt, counts=ct, **{k: v for k, v in kw.items() if k != "group_boxes"})[0]
    else:
        assert boxes.shape[0] == 1 and counts is None
        prob = G.differentiable_nms(st[0], overlaps.iou(bt[0], bt[0]), **kw)[2][None]
    (prob * wt).sum().backward()
    return prob.detach(), st.grad, bt.grad


def check_layer(tag, got, r):
    keep = ~r["skip"]
    ratio = bound_ratio(got[keep], r["ref"][keep], r["bound"][keep])
    print("layer %-44s error / bound %.3f  (largest |grad| %.3e, %d boxes left out)" % (tag, ratio, float(np.abs(r["ref"]).max()), int(r["skip"].sum())))
    assert ratio <= 1.0, tag


@pytest.mark.parametrize("n,mode,entry", LAYER_PARAMS, ids=["%d-%s-%s" % c for c in LAYER_PARAMS])
def test_layer_box_gradient(G, n, mode, entry):
    boxes, scores, w, r = layer_case(n, mode)
    kw = MODE_KW[mode]
    prob, gs, gb = run_entry(G, entry, boxes[None], scores[None], w[None], kw)
    assert gb is not None, "boxes.grad is missing"
    assert tuple(gb.shape) == (1, n, 4) and bool(torch.isfinite(gb).all())
    check_layer("%s n=%d %s" % (entry, n, mode), gb[0].cpu().numpy(), r)
    # prob and dL/dscores are the bits of the call without a box gradient
    prob0, gs0, none = run_entry(G, entry, boxes[None], scores[None], w[None], kw, box_grad=False)
    assert none is None
    assert torch.equal(prob, prob0), "prob changed"
    assert torch.equal(gs, gs0), "grad_scores changed"
    np.testing.assert_allclose(prob[0].cpu().numpy(), r["prob"], atol=1e-4, rtol=0)
    # the same inputs give the same bits
    assert torch.equal(gb, run_entry(G, entry, boxes[None], scores[None], w[None], kw)[2])


@pytest.mark.parametrize("n,mode", LAYER_CASES, ids=["%d-%s" % c for c in LAYER_CASES])
def test_two_call_box_gradient_against_its_own_cotangent(G, n, mode):
    """The bound of test_layer_box_gradient carries, outside masked-linear, the tolerance of the matrix gradient, which dwarfs the
    box-gradient arithmetic's own error there.  This holds that arithmetic alone, in every mode: boxes.grad against the float64 closed
    form contracted with the float32 matrix gradient the layer ACTUALLY produced (retained on the way), to the bound without that term."""
    from groomed_nms_amd import overlaps
    boxes, scores, w, _ = layer_case(n, mode)
    bt, st = dev(boxes).requires_grad_(True), dev(scores).requires_grad_(True)
    m = overlaps.iou(bt, bt)
    m.retain_grad()
    prob = G.differentiable_nms(st, m, **MODE_KW[mode])[2]
    (prob * dev(w)).sum().backward()
    g = m.grad.cpu().numpy()
    assert g.any()
    f = closed_form_self(boxes, g)
    ratio = bound_ratio(bt.grad.cpu().numpy(), f["d"], f["bound"])
    print("layer two_call n=%d %-10s against its own cotangent: error / bound %.3f (%d non-zero cotangents)" % (n, mode, ratio, int((g != 0).sum())))
    assert ratio <= 1.0


@pytest.mark.parametrize("n,mode", SPARSE_PARAMS, ids=["%d-%s" % c for c in SPARSE_PARAMS])
def test_sparse_route_members_are_the_dense_route_s_bits(G, n, mode):
    from groomed_nms_amd import groomed_nms as GN
    boxes, scores, w, r = layer_case(n, mode)
    kw = MODE_KW[mode]
    sparse = run_entry(G, "with_iou2d", boxes[None], scores[None], w[None], kw)[2][0].cpu().numpy()
    assert GN.BOX_GRAD_ROUTE == "auto"
    GN.BOX_GRAD_ROUTE = "dense"
    try:
        dense = run_entry(G, "with_iou2d", boxes[None], scores[None], w[None], kw)[2][0].cpu().numpy()
        dense_fb = run_entry(G, "from_boxes", boxes[None], scores[None], w[None], kw)[2][0].cpu().numpy()
    finally:
        GN.BOX_GRAD_ROUTE = "auto"
    assert dense.tobytes() == dense_fb.tobytes(), "the dense route with the kept matrix and with the rebuilt one differ"
    members = ~r["heads"]
    assert members.sum() > 0 and r["heads"].sum() > 0
    assert np.array_equal(sparse[members], dense[members]), "a member's gradient has one term: the two routes must give the same bits"
    assert sparse[members].any()
    check_layer("dense route n=%d %s" % (n, mode), dense, r)           # (the heads of the sparse route: test_layer_box_gradient)


@pytest.mark.parametrize("entry", ["with_iou2d", "from_boxes"])
@pytest.mark.parametrize("mode", ["default", "unmasked"])
@pytest.mark.parametrize("n", [37, 500])
def test_ragged_counts_with_an_empty_image(G, n, mode, entry):
    counts = [n, 0, n - n // 3]
    boxes = np.zeros((3, n, 4), np.float32)
    scores = np.zeros((3, n), np.float32)
    w = np.zeros((3, n), np.float32)
    refs = []
    for b, c in enumerate(counts):
        bx, sc, ww = layer_inputs(n, mode, image=b + 1)
        boxes[b], scores[b], w[b] = bx, sc, ww
        refs.append(reference_of(bx[:c], sc[:c], ww[:c], mode))
    prob, gs, gb = run_entry(G, entry, boxes, scores, w, MODE_KW[mode], counts=counts)
    gb = gb.cpu().numpy()
    for b, c in enumerate(counts):
        assert not gb[b, c:].any(), "boxes behind counts[b] get exactly 0"
        if c:
            check_layer("%s n=%d %s image %d (%d boxes)" % (entry, n, mode, b, c), gb[b, :c], refs[b])
    prob0, gs0, _ = run_entry(G, entry, boxes, scores, w, MODE_KW[mode], box_grad=False, counts=counts)
    assert torch.equal(prob, prob0) and torch.equal(gs, gs0)


@pytest.mark.parametrize("entry", ["with_iou2d", "from_boxes"])
@pytest.mark.parametrize("mode", ["default", "unmasked"])
def test_unaligned_boxes_view(G, mode, entry):
    n = 500
    boxes, scores, w, r = layer_case(n, mode)
    base = torch.zeros(4 * n + 1, device="cuda")
    base[1:] = dev(boxes).reshape(-1)
    base.requires_grad_(True)
    view = base[1:].view(1, n, 4)
    assert view.data_ptr() % 16 == 4
    st = dev(scores[None]).requires_grad_(True)
    if entry == "with_iou2d":
        prob = G.differentiable_nms_with_iou2d_batched(st, view, **MODE_KW[mode])[0]
    else:
        prob = G.differentiable_nms_from_boxes_batched(st, view, **{k: v for k, v in MODE_KW[mode].items() if k != "group_boxes"})[0]
    (prob * dev(w[None])).sum().backward()
    assert float(base.grad[0]) == 0.0
    check_layer("unaligned %s %s" % (entry, mode), base.grad[1:].view(n, 4).cpu().numpy(), r)
    prob0, gs0, _ = run_entry(G, entry, boxes[None], scores[None], w[None], MODE_KW[mode], box_grad=False)
    assert torch.equal(prob.detach(), prob0) and torch.equal(st.grad, gs0)


@pytest.mark.parametrize("mode", ["default", "unmasked"])
def test_forward_and_backward_in_a_graph(G, mode):
    """captured once, replayed on other contents: the replay's bits are eager's (sparse route: default; dense route: unmasked)"""
    n = 500
    kw = MODE_KW[mode]
    cases = [layer_inputs(n, mode, image=7), layer_inputs(n, mode, image=8)]
    eager = [run_entry(G, "with_iou2d", b[None], s[None], w[None], kw) for b, s, w in cases]
    bt = dev(cases[0][0][None]).requires_grad_(True)
    st = dev(cases[0][1][None]).requires_grad_(True)
    wt = dev(cases[0][2][None])

    def step():
        prob = G.differentiable_nms_with_iou2d_batched(st, bt, **kw)[0]
        return (prob,) + torch.autograd.grad((prob * wt).sum(), (st, bt))
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
            bt.copy_(dev(cases[which][0][None]))
            st.copy_(dev(cases[which][1][None]))
            wt.copy_(dev(cases[which][2][None]))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[which]):
            assert torch.equal(got.detach(), want), "the replay differs from the eager run"
