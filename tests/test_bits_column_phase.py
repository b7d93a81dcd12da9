"""The row-buffer bit-matrix kernel (bitmask_boxes_kernel<4, KBW, true>).  With two rank blocks per workgroup the columns' ranks are gathered
behind the hull computation, held in registers and waited for only where the first finished word is parked.  launch_bitmask_boxes takes that
route for 1024 < N <= 4096 with B * ceil(N / 64) > 256 (the CU count) and B * ceil(N / 64) * ceil(N / 256) >= 2048; the smallest shapes that
do: B = 9, N = 2048 (288 rank blocks, an even number per image) and B = 8, N = 2112 (33 rank blocks: the image's last workgroup has one block,
and the last column chunk is partial).  B = 4, N = 4096 has exactly 256 rank blocks: one block per workgroup, the ranks stashed in LDS -- the
same body.

Everything the one-call entry (gnms_forward_with_iou2d) returns is compared BIT FOR BIT with the matrix-in route on the same inputs
(overlaps.iou_batched -> differentiable_nms_batched: its threshold bits come from bitmask_kernel, which reads the matrix) and, on plain
inputs, with the CPU oracle on two images of the batch (tolerance 0: the default mode is bit-exact)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(9, 2048), (8, 2112)]
THRESHOLDS = [-1.0, 0.4, 1.0]


@pytest.fixture(scope="module")
def G():
    import groomed_nms_amd as g
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return g


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _grad_prob(N):
    return np.linspace(-1, 2, N).astype(np.float32)                  # dL/dprob, the same bits for the GPU routes and the oracle


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _both_routes(G, boxes, scores, counts, thr):
    """(outputs[:6], grad_scores) of the one-call entry and of the matrix-in route."""
    from groomed_nms_amd import overlaps
    B, N = scores.shape
    bt = torch.from_numpy(boxes).cuda()
    ct = None if counts is None else torch.tensor(counts, dtype=torch.int32).cuda()
    w = torch.from_numpy(_grad_prob(N)).cuda().repeat(B, 1)
    res = []
    for fn in (lambda s: G.differentiable_nms_with_iou2d_batched(s, bt, counts=ct, nms_threshold=thr),
               lambda s: G.differentiable_nms_batched(s, overlaps.iou_batched(bt), counts=ct, nms_threshold=thr)):
        s = torch.from_numpy(scores).cuda().requires_grad_(True)
        out = fn(s)
        (out[0] * w).sum().backward()
        res.append(([o.detach().clone() for o in out[:6]], s.grad.clone()))
        del out
    return res


def _assert_same(res, tag):
    (o1, g1), (o2, g2) = res
    names = ("prob", "order", "valid", "invalid", "nvalid", "ninvalid")
    for name, a, b in zip(names, o1, o2):
        assert torch.equal(_bits(a), _bits(b)), (tag, name)
    assert torch.equal(_bits(g1), _bits(g2)), (tag, "grad_scores")


def _assert_oracle(O, boxes, scores, thr, res, images, tag):
    (o, g), _ = res
    N = scores.shape[1]
    w = _grad_prob(N)
    for b in images:
        m = O.iou2d(boxes[b], boxes[b])
        ref = O.differentiable_nms(scores[b], m, nms_threshold=thr, grad_prob=w)
        assert np.array_equal(o[0][b].cpu().numpy(), ref["prob"]), (tag, b, "prob")
        assert o[1][b].tolist() == ref["order"].tolist(), (tag, b, "order")
        assert o[2][b, :int(o[4][b])].tolist() == list(ref["valid"]), (tag, b, "valid")
        assert sorted(o[3][b, :int(o[5][b])].tolist()) == sorted(ref["invalid"].tolist()), (tag, b, "invalid")
        assert np.array_equal(g[b].cpu().numpy(), ref["grad_scores"]), (tag, b, "grad_scores")


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_two_block_route_full_images(G, O, B, N, kind, thr):
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(300 + N, B, N, kind)
    res = _both_routes(G, boxes, scores, None, thr)
    _assert_same(res, (B, N, kind, thr))
    assert thr >= 1.0 or int(res[0][0][4].sum()) > 0                # (threshold 1: every box leads a group of its own and none is valid)
    _assert_oracle(O, boxes, scores, thr, res, (0, B - 1), (B, N, kind, thr))


def _ragged_counts(B, N):
    c = [N, N - 200, 65, 0, N - 1, 64, 1, N - 63, 1025]
    return c[:B]


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_two_block_route_ragged_counts(G, B, N, thr):
    """Images of N - 200 and 65 boxes end inside a column chunk; one image has no box at all."""
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(400 + N, B, N, "clustered")
    res = _both_routes(G, boxes, scores, _ragged_counts(B, N), thr)
    _assert_same(res, (B, N, thr))
    assert res[0][0][4].tolist()[3] == 0 and (thr >= 1.0 or int(res[0][0][4].sum()) > 0)


def _spoil(boxes):
    """Boxes that are not plain: zero area, x2 < x1, a NaN coordinate -- the exact-division fallback, and cols_ok == false in their chunks."""
    boxes = boxes.copy()
    B, N, _ = boxes.shape
    rng = np.random.default_rng(7)
    for b in range(B):
        if b == 1:
            continue                                                  # (one image stays plain beside the others)
        idx = rng.choice(N, 24, replace=False)
        for k, i in enumerate(idx):
            if k % 3 == 0:
                boxes[b, i, 2] = boxes[b, i, 0]                       # zero area
            elif k % 3 == 1:
                boxes[b, i, 0], boxes[b, i, 2] = boxes[b, i, 2] + 1.0, boxes[b, i, 0]   # x2 < x1
            else:
                boxes[b, i, k % 4] = np.nan
    return boxes


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_two_block_route_boxes_that_are_not_plain(G, B, N, thr):
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(500 + N, B, N, "uniform")
    boxes = _spoil(boxes)
    for counts in (None, _ragged_counts(B, N)):
        _assert_same(_both_routes(G, boxes, scores, counts, thr), (B, N, thr, counts is None))


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_one_block_route_with_the_stash(G, O, thr):
    """B = 4, N = 4096: exactly 256 rank blocks, one per workgroup (KBW = 1, the ranks wait in LDS)."""
    from groomed_nms_amd import synthetic
    B, N = 4, 4096
    for kind in ("uniform", "clustered"):
        boxes, scores = synthetic.batch_2d(600, B, N, kind)
        res = _both_routes(G, boxes, scores, None, thr)
        _assert_same(res, (kind, thr))
        _assert_oracle(O, boxes, scores, thr, res, (0, B - 1), (kind, thr))
    boxes = _spoil(boxes)
    _assert_same(_both_routes(G, boxes, scores, [N, N - 200, 65, 0], thr), ("spoiled, ragged", thr))
