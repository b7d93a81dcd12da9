"""The KITTI evaluation on the GPU (groomed_nms_amd.kitti_eval.evaluate, csrc/kitti_eval.hip) against the Python restatement of the
devkit in test_kitti_eval_host.py.  Overlap matrices within 1e-12 (the bound of the project's float64 exact-IoU list), n_gt / tp / fp /
fn exact, thresholds bit-equal, precision ==, aos within 1e-9 (every case stays below 2000 true and false positives per curve:
2000 * 2000 * 2^-53 = 4.4e-10 for the order of summation).  Every seed satisfies the margin condition (checked by the restatement, on
the CPU as well: test_committed_seeds_have_margin)."""
import io
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import test_kitti_eval_host as H

pytestmark = pytest.mark.gpu

CASES = {"mixed": (H.scene_mixed, [H.MAIN, H.SIDE, H.grid(30, 0.3), H.grid(45, 0.5)]), "words": (H.scene_words, [H.MAIN]),
         "many": (H.scene_many, [H.MAIN]), "rules": (H.scene_rules, [H.MAIN, H.SIDE]), "no3d": (H.scene_no3d, [H.MAIN])}
_cache = {}


def case(name):
    """(scene, variants, reference, device results with intermediates), computed once"""
    if name not in _cache:
        from groomed_nms_amd import kitti_eval as K
        make, variants = CASES[name]
        seed, scene, ref = H.with_margin(make, variants, H.COMMITTED_SEEDS[make.__name__])
        assert seed == H.COMMITTED_SEEDS[make.__name__]
        got = K.evaluate(*H.pack(scene), variants=variants, return_intermediates=True)
        _cache[name] = (scene, variants, ref, got)
    return _cache[name]


def compare(scene, ref, got):
    sw, overlaps, per_variant = ref
    assert len(got) == len(per_variant)
    for metric in range(3):                                                      # overlap matrices: every entry the restatement used
        for img, memo in enumerate(overlaps[metric]):
            m = got[0]["overlaps"][img][metric]
            assert m.shape == (len(scene[img][1]), len(scene[img][0]))
            for (j, i, criterion), want in memo.memo.items():
                if criterion == -1 and scene[img][0][i].type.lower() == "dontcare":
                    continue                                                     # (never read by the devkit: the row's ignored_gt is -1)
                assert abs(m[j, i] - want) <= 1e-12 or (math.isnan(want) and math.isnan(m[j, i])), (metric, img, j, i, m[j, i], want)
    for g, curves in zip(got, per_variant):
        assert g["compute_aos"] == sw.compute_aos
        assert g["eval_image"].tolist() == sw.eval_image and g["eval_ground"].tolist() == sw.eval_ground and g["eval_3d"].tolist() == sw.eval_3d
        positives = 0
        for c in range(3):
            for metric in range(3):
                for d in range(3):
                    key = (c, metric, d)
                    if key not in curves:                                        # a curve that is off
                        assert not g["precision"][key].any() and g["n_thresholds"][key] == 0
                        continue
                    r = curves[key]
                    n = len(r.thresholds)
                    assert g["n_gt"][key] == r.n_gt and g["n_thresholds"][key] == n, key
                    assert g["thresholds"][key][:n].tolist() == r.thresholds, key
                    assert g["tp"][key][:n].tolist() == r.tp and g["fp"][key][:n].tolist() == r.fp and g["fn"][key][:n].tolist() == r.fn, key
                    assert all(t + f > 0 for t, f in zip(r.tp, r.fp)), "0 / 0 at a threshold: no test may depend on it"
                    positives = max([positives] + [t + f for t, f in zip(r.tp, r.fp)])
                    assert g["precision"][key].tolist() == r.precision, key
                    if metric == 0:
                        if r.aos is None:
                            assert not g["aos"][c, d].any()
                        else:
                            assert np.abs(g["aos"][c, d] - np.array(r.aos)).max() <= 1e-9, key
        assert positives <= 2000


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_restatement(name):
    scene, variants, ref, got = case(name)
    compare(scene, ref, got)


def test_case_shapes_are_what_they_claim():
    scene, _, (sw, _, (curves,)), got = case("words")
    assert [len(d) for _, d in scene] == [70, 130, 0] and sw.eval_image == [True, False, False]          # Cyclist objects, never detected
    assert any(len(r.thresholds) == 5 for r in curves.values())
    scores = [d.thresh for d in scene[1][1]]
    assert len(set(scores)) < len(scores)                                        # ties
    _, _, (_, _, (curves,)), got = case("many")
    assert len(curves[(0, 0, 1)].thresholds) == 41 and got[0]["n_thresholds"][0, 0, 1] == 41 and 250 <= curves[(0, 0, 1)].tp[-1] <= 400
    scene, _, (_, _, (curves, _)), _ = case("rules")
    assert curves[(0, 1, 1)].fp != curves[(0, 0, 1)].fp                          # the stuff areas act on the image metric only
    _, _, (sw, _, _), got = case("no3d")
    assert sw.eval_ground == [True, False, True] and sw.eval_3d == [True, False, False]
    _, _, (_, _, per_variant), _ = case("mixed")
    assert per_variant[0][(0, 0, 2)].n_gt != per_variant[2][(0, 0, 2)].n_gt      # max_depth changes n_gt


def test_alpha_minus_10_switches_orientation_off():
    from groomed_nms_amd import kitti_eval as K
    scene = H.pin_b_scene()
    scene[1][1][1].alpha = -10.0
    got = K.evaluate(*H.pack(scene), variants=[H.MAIN], return_intermediates=True)
    ref = H.ref_eval(scene, [H.MAIN])
    compare(scene, ref, got)
    assert not got[0]["compute_aos"] and not got[0]["aos"].any()
    assert got[0]["precision"][0, 0, 0][:3].tolist() == [1.0, 2.0 / 3.0, 0.0]     # the hand-worked pin (b)


def test_variants_in_one_call_equal_single_calls_and_repeat_bit_for_bit():
    from groomed_nms_amd import kitti_eval as K
    scene, variants, _, got = case("mixed")
    packed = [torch.from_numpy(a).cuda() if a.dtype == np.float64 else a for a in H.pack(scene)]     # device rows, host int32 offsets
    again = K.evaluate(packed[0], packed[1].astype(np.int64), packed[2], packed[3], variants=variants, return_intermediates=True)
    keys = ("precision", "aos", "n_gt", "thresholds", "n_thresholds", "tp", "fp", "fn")
    for a, b in zip(got, again):
        for k in keys:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["overlaps"], b["overlaps"]))
    for v, variant in enumerate(variants):
        single = K.evaluate(*packed, variants=[variant], return_intermediates=True)[0]
        for k in keys:
            assert np.array_equal(single[k], got[v][k], equal_nan=True), (v, k)


def test_limits_raise_and_empty_input():
    from groomed_nms_amd import kitti_eval as K
    with pytest.raises(ValueError, match="limit"):
        K.evaluate(np.zeros((513, 14)), [0, 513], np.zeros((1, 15)), [0, 1])
    r = K.evaluate(np.zeros((0, 14)), np.zeros(3, np.int32), np.zeros((0, 15)), np.zeros(3, np.int32), return_intermediates=True)[0]
    assert not r["precision"].any() and not r["eval_image"].any() and r["compute_aos"]
    # the documented limits themselves: 512 detections against 64 ground truths in one image (one curve of the restatement)
    scene, r = H.limits_case()
    g = K.evaluate(*H.pack(scene), variants=[H.SIDE], return_intermediates=True)[0]
    n = len(r.thresholds)
    assert g["n_gt"][0, 0, 1] == r.n_gt and g["thresholds"][0, 0, 1][:n].tolist() == r.thresholds and n > 20
    assert g["tp"][0, 0, 1][:n].tolist() == r.tp and g["fp"][0, 0, 1][:n].tolist() == r.fp and g["fn"][0, 0, 1][:n].tolist() == r.fn
    assert g["precision"][0, 0, 1].tolist() == r.precision


def test_run_kitti_eval_and_verbose(tmp_path):
    from groomed_nms_amd import kitti_eval as K
    scene = case("rules")[0]
    results, labels = H.write_folders(scene, str(tmp_path / "kitti" / "validation"))
    lbls = ["Car", "Pedestrian", "Cyclist"]
    read_back = H.rounded6(scene)
    want = {}
    for name, variant in (("main", H.MAIN), ("side", H.SIDE)):
        _, _, (curves,) = H.ref_eval(read_back, [variant], margin=0.0)
        d = {}
        for (c, metric, diff), r in sorted(curves.items()):
            for key, curve in ((("det_2d_", "gr_", "det_3d_")[metric], r.precision),) + ((("or_", r.aos),) if r.aos is not None else ()):
                rounded = [float("%f" % x) for x in curve]
                d.setdefault(key + H.CLASS_NAMES[c], [None] * 3)[diff] = float(np.mean(rounded[1:41]))
        want[name] = d
    got = K.run_kitti_eval(results, labels, lbls, variant=K.MAIN, use_40=True)
    assert set(got) == set(want["main"]) and len(got) == 12
    for k in got:
        assert np.abs(np.array(got[k]) - np.array(want["main"][k])).max() <= 1e-6 + 1e-12, k      # aos within 1e-9 may round to the next %f step
        if not k.startswith("or_"):
            assert list(got[k]) == want["main"][k], k
    assert os.path.exists(os.path.join(results, "stats_car_detection_3d.txt"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        obj = K.evaluate_kitti_results_verbose(str(tmp_path), "kitti", os.path.join(results, "data"), split_name=os.path.join("validation"),
                                               test_iter=7, conf={"lbls": lbls}, use_logging=False, fast=True)
    out = buf.getvalue().splitlines()
    assert set(obj) == {"main", "side"} and obj["main"] == got
    e, m, h = got["det_2d_car"]
    assert "test_iter 7 car 2d  --> easy: {:0.4f}, mod: {:0.4f}, hard: {:0.4f}".format(e, m, h) in out
    e, m, h = obj["side"]["gr_pedestrian"]
    assert "test_iter 7 pedestrian bev --> easy: {:0.4f}, mod: {:0.4f}, hard: {:0.4f}".format(e, m, h) in out
    assert sum(line.startswith("test_iter 7 ") for line in out) == 24 and out.count("") == 2
    for k in obj["side"]:
        if not k.startswith("or_"):
            assert list(obj["side"][k]) == want["side"][k], k
