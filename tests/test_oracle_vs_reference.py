"""The oracle against the reference on inputs the golden fixtures of the other files do not hold.

`tests/golden/oracle_vs_reference.npz` holds, for every case below, inputs drawn from the case's seed and what the reference computed on
them (tests/golden/make_golden.py::make_oracle_vs_reference: lib/groomed_nms.py:10 differentiable_nms with autograd, lib/core.py:480 iou,
...) -- sizes, generators, modes and pruning methods beyond the other fixtures.  Tolerances: the overlap matrix bit for bit; probabilities
and gradients 2e-6 (the reference multiplies an N x N inversion matrix where the oracle evaluates the closed form: different summation
order); valid / invalid index SETS equal (the order among exactly tied probabilities is implementation-defined in torch.sort)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


CASES = [   # (seed, N, generator, kwargs)
    (101, 37, "uniform", {}),
    (102, 129, "clustered", {}),
    (103, 300, "clustered", dict(nms_threshold=0.55, group_size=3)),
    (104, 200, "uniform", dict(pruning_method="sigmoidal", temperature=0.1)),
    (105, 160, "clustered", dict(pruning_method="soft_nms", temperature=0.3, valid_box_prob_threshold=0.1)),
    (106, 150, "clustered", dict(mask_group_boxes=False)),
    (107, 120, "clustered", dict(group_boxes=False)),
    (108, 257, "clustered", dict(return_sorted_prob=True, nms_threshold=0.3)),
    (109, 2, "uniform", {}),
    (110, 1, "uniform", {}),
]


@pytest.mark.parametrize("seed,N,kind,kw", CASES)
def test_oracle_equals_the_reference_on_fresh_inputs(ref, O, seed, N, kind, kw):
    k = "%d/" % seed
    boxes, scores, w = ref[k + "boxes"], ref[k + "scores"], ref[k + "w"]
    assert boxes.shape == (N, 4)
    iou_ref = ref[k + "iou"]
    iou_orc = O.iou2d(boxes, boxes)
    assert np.array_equal(iou_ref, iou_orc), "overlap matrix differs from lib/core.py iou"
    got = O.differentiable_nms(scores, iou_orc, grad_prob=w, **kw)
    np.testing.assert_allclose(got["prob"], ref[k + "prob"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got["grad_scores"], ref[k + "grad_scores"], rtol=0, atol=2e-6)
    assert set(int(i) for i in got["valid"]) == set(int(i) for i in ref[k + "valid"]), "valid_boxes_index"
    assert set(int(i) for i in got["invalid"]) == set(int(i) for i in ref[k + "invalid"]), "invalid_boxes_index"


@pytest.mark.parametrize("seed,N,clustered", [(201, 23, False), (202, 96, True), (203, 170, True)])
def test_oracle_3d_overlaps_equal_the_reference_on_fresh_inputs(ref, O, seed, N, clustered):
    """lib/math_3d.py get_corners_of_cuboid + lib/core.py:352 iou3d_approximate, both methods, and what the callers feed the
    layer (0.5 * (1 + giou), lib/loss/rpn_3d.py:781).  Corners 2e-5 (sin/cos rounding differs between libm and torch); the
    overlap arithmetic from the REFERENCE's corners 1e-6 -- the same split tests/test_oracle_golden.py makes."""
    k = "%d/" % seed
    p, cn = ref[k + "params"], ref[k + "corners"]
    assert p.shape == (N, 7)
    np.testing.assert_allclose(O.corners_of_cuboid(p), cn, atol=2e-5, rtol=1e-6)
    for method in ("normal", "generalized"):
        ob, o3 = O.iou3d_approximate(cn, cn, generalized=(method == "generalized"))
        np.testing.assert_allclose(ob, ref[k + method + "/bev"], atol=1e-6, rtol=1e-6)
        np.testing.assert_allclose(o3, ref[k + method + "/iou3d"], atol=1e-6, rtol=1e-6)
    # rectangular call: a against b
    ob, o3 = O.iou3d_approximate(cn, ref[k + "corners_b"], generalized=True)
    np.testing.assert_allclose(ob, ref[k + "rect/bev"], atol=1e-6, rtol=1e-6)
    np.testing.assert_allclose(o3, ref[k + "rect/iou3d"], atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("seed,N,kind", [(301, 1, "uniform"), (302, 75, "clustered"), (303, 400, "clustered"), (304, 250, "uniform")])
def test_oracle_classic_nms_equals_the_reference_on_fresh_inputs(ref, O, seed, N, kind):
    """lib/nms/py_cpu_nms.py:10 and lib/nms_others.py:119 girshick_nms on seeded detections: kept index LISTS equal."""
    from oracle import nms_others_oracle as NO
    k = "%d/" % seed
    dets = ref[k + "dets"]
    assert dets.shape == (N, 5)
    for thr in (0.3, 0.5, 0.75):
        want = [int(i) for i in ref[k + "py_cpu_nms/%g" % thr]]
        assert O.classic_nms(dets, thr, rule="py") == want
        assert O.classic_nms(dets, thr, rule="gpu") == want      # '>' and 'not <=' differ only at equality / NaN
        for shift in (0, 1):
            assert list(NO.girshick_nms(dets, thr, shift=shift)) == [int(i) for i in ref[k + "girshick_nms/%g/%d" % (thr, shift)]]


@pytest.mark.parametrize("seed,N,temp", [(401, 12, 0.01), (402, 33, 0.002), (403, 64, 0.001)])
def test_oracle_soft_sort_equals_the_reference_on_fresh_inputs(ref, O, seed, N, temp):
    """lib/groomed_nms.py:131 soft_sort on score-sorted inputs (the only inputs on which the reference's layer terminates with
    soft sorting, see tests/golden/make_golden.py): permutation matrix, soft scores and the row-mixed overlap matrix, 1e-5."""
    k = "%d/" % seed
    s, m = ref[k + "scores"], ref[k + "iou"]
    assert s.shape == (N,)
    oss, oC, osm = O.soft_sort(s, m, temp)
    np.testing.assert_allclose(oC, ref[k + "perm"], atol=1e-5)
    np.testing.assert_allclose(oss, ref[k + "soft_scores"], atol=1e-5)
    np.testing.assert_allclose(osm, ref[k + "soft_iou"], atol=1e-5)
