"""Host side of the device-resident validation tail (groomed_nms_amd.kitti_results, csrc/kitti_rows.hip): the golden file is
consistent with the devkit's parser, arguments are validated before any device call, the class table follows the devkit's strcasecmp,
and the new symbols are declared.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import Golden, ROOT

from groomed_nms_amd import _lib, kitti_eval as K, kitti_results as R


@pytest.fixture(scope="module")
def golden():
    return Golden("kitti_rows.npz")


def test_golden_text_parses_to_its_rows(golden):
    assert golden.cases() == ["two_passes", "wave_boundary"]
    for c in golden.cases():
        per_image = [[K._det_row(v) for v in K._parse(str(t), 16, -1, K._det_class)] for t in golden[c + "/text"]]
        rows, offsets = K._pack(per_image, K.DET_COLS)
        want = golden[c + "/rows"]
        assert rows.shape == want.shape and np.array_equal(rows, want) and np.array_equal(np.signbit(rows), np.signbit(want))
        assert offsets.tolist() == golden[c + "/offsets"].tolist()
        assert int(golden[c + "/redraws"]) <= 20


def test_golden_cases_hold_what_they_are_for(golden):
    c = "wave_boundary"
    det, counts, off = golden[c + "/det"], golden[c + "/counts"], golden[c + "/offsets"]
    assert det.shape == (3, 70, 14) and det.dtype == np.float32 and counts.tolist() == [0, 70, 37] and int(golden[c + "/nms_topN_post"]) == 50
    b, k = golden[c + "/exact"].tolist()
    assert float(det[b, k, 4]) == float(golden[c + "/score_thres"]) and k < counts[b]           # the score on the threshold: dropped
    assert len(set(map(bytes, golden[c + "/p2"]))) == 3                                         # a different p2 per image
    assert list(golden[c + "/lbls"]) == ["Car", "Pedestrian", "Cyclist", "Van"] and (golden[c + "/rows"][:, 0] == -1).any()
    assert (golden[c + "/rows"][:, 9] < 0).any()
    c = "two_passes"
    off = golden[c + "/offsets"].tolist()
    assert golden[c + "/counts"].tolist()[1] > 0 and off[1] == off[2] == off[3] < off[4]        # every row of image 1 is dropped


def test_class_table_follows_strcasecmp():
    assert R.class_table(["Car", "Pedestrian", "Cyclist"]).tolist() == [0, 1, 2]
    assert R.class_table(["cyclist", "VAN", "CAR", "pedestrian", "Person_sitting", "Cars"]).tolist() == [2, -1, 0, 1, -1, -1]
    assert R.class_table(["Car"]).dtype == np.int32
    for bad in ([], ["Car"] * 17, ["Car", ""], ["Car", "Person sitting"], ["Car", 3]):
        with pytest.raises(ValueError):
            R.class_table(bad)


def test_python_arguments_are_validated_before_any_device_call():
    with pytest.raises(ValueError):
        R.KittiResults([], 0.75, 50, 4, 200, device="cpu")
    with pytest.raises(ValueError):
        R.KittiResults(["Car"], 0.75, -1, 4, 200, device="cpu")
    with pytest.raises(ValueError):
        R.KittiResults(["Car"], float("nan"), 50, 4, 200, device="cpu")
    with pytest.raises(ValueError):
        R.KittiResults(["Car"], 0.75, 50, 4, 2 ** 31, device="cpu")
    with pytest.raises(_lib.GnmsError):                                  # no CPU fallback
        R.KittiResults(["Car"], 0.75, 50, 4, 200, device="cpu")
    with pytest.raises(ValueError):
        R.round6(torch.zeros(3, dtype=torch.float32))
    with pytest.raises(ValueError):
        R.round6(np.zeros(3))
    with pytest.raises(ValueError):
        R.round6(torch.zeros(3, dtype=torch.float64), count=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.GnmsError):
        R.round6(torch.zeros(3, dtype=torch.float64))
    for conf in (dict(lbls=["Car"], score_thres=0.75, nms_topN_post=50, has_un=True),
                 dict(lbls=["Car"], score_thres=0.75, nms_topN_post=50, use_un_for_score=True)):
        with pytest.raises(NotImplementedError):
            R.KittiResults.from_conf(conf, 4)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                                       # host memory: a call that got past the checks would fault on it
    p = ctypes.addressof(buf)

    def append(det=p, cols=14, counts=p, p2_inv=p, B=1, Kmax=1, topn=50, class_ids=p, n_lbls=3, scratch=p, rows=p, lbl=p, cap=4, offsets=p,
               n_off=2, base=0, state=p):
        return lib.gnms_kitti_rows_append(det, cols, counts, p2_inv, B, Kmax, topn, 0.75, class_ids, n_lbls, scratch, rows, lbl, cap, offsets, n_off,
                                          base, state, None)
    for kw, word in ((dict(cols=13), "14 columns"), (dict(Kmax=-1), "negative"), (dict(B=-1), "negative"), (dict(n_lbls=0), "n_lbls"),
                     (dict(n_lbls=17), "n_lbls"), (dict(topn=-1), "nms_topN_post"), (dict(det=None), "null"), (dict(counts=None), "null"),
                     (dict(p2_inv=None), "null"), (dict(class_ids=None), "null"), (dict(rows=None), "null"), (dict(offsets=None), "null"),
                     (dict(state=None), "null"), (dict(scratch=None), "null"), (dict(cap=-1), "capacity"), (dict(n_off=0), "n_offsets"),
                     (dict(base=-1), "image_base")):
        assert append(**kw) == -1, kw
        assert word in lib.gnms_last_error().decode(), (kw, lib.gnms_last_error())
    assert lib.gnms_round6(None, p, 4, None, None) == -1 and "null" in lib.gnms_last_error().decode()
    assert lib.gnms_round6(p, None, 4, None, None) == -1
    assert lib.gnms_round6(p, p, -1, None, None) == -1 and "negative" in lib.gnms_last_error().decode()
    assert lib.gnms_round6(None, None, 0, None, None) == 0               # nothing to do, nothing launched


def test_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    build = open(os.path.join(ROOT, "groomed_nms_amd", "build.py")).read()
    for name in ("gnms_kitti_rows_append", "gnms_round6"):
        assert "int %s(" % name in header and name in _lib.EXPORTED_SYMBOLS
    assert '"kitti_rows.hip"' in build
    assert R.MAX_LBLS == 16 and "#define GNMS_KITTI_ROWS_MAX_LBLS 16" in header and "#define GNMS_KITTI_ROWS_STATE_WORDS 8" in header
    import groomed_nms_amd as G
    assert G.KittiResults is R.KittiResults and G.round6 is R.round6 and G.evaluate_detections is K.evaluate_detections
