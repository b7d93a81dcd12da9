"""Detections -> the rows the devkit would parse -> AP on the device (groomed_nms_amd.kitti_results, csrc/kitti_rows.hip).

Everything is compared EXACTLY (== and the sign bit): the goldens come from the reference's own functions inside a guard band
(tests/golden/make_kitti_rows_golden.py) in which a last-ulp difference of matmul / atan2 cannot change a row; the rounding is compared
with float('%.6f' % v) computed here; the end-to-end test compares with the file route (kitti_io writes, kitti_eval.load_results reads),
which holds no code of kitti_results."""
import os

import numpy as np
import pytest
import torch

from conftest import Golden

pytestmark = pytest.mark.gpu

_golden = None
_cache = {}


def golden():
    global _golden
    if _golden is None:
        _golden = Golden("kitti_rows.npz")
    return _golden


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def inputs(c):
    from groomed_nms_amd import detect
    g = golden()
    det = torch.from_numpy(g[c + "/det"]).cuda()
    counts = torch.from_numpy(g[c + "/counts"]).cuda()
    p2_inv = detect.camera_constants(g[c + "/p2"], 1.0, (1, 1), det.shape[0])[0]
    kw = dict(lbls=[str(s) for s in g[c + "/lbls"]], score_thres=float(g[c + "/score_thres"]), nms_topN_post=int(g[c + "/nms_topN_post"]))
    return det, counts, p2_inv, kw


def collect(c, per_image=False, capacity=None, max_images=None):
    from groomed_nms_amd import KittiResults
    det, counts, p2_inv, kw = inputs(c)
    B = det.shape[0]
    r = KittiResults(max_images=B if max_images is None else max_images, capacity_rows=B * kw["nms_topN_post"] if capacity is None else capacity, **kw)
    if per_image:
        for b in range(B):
            r.append(det[b:b + 1], counts[b:b + 1], p2_inv[b:b + 1])
    else:
        r.append(det, counts, p2_inv)
    return r


def one_batch(c):
    """(accumulator, rows on the host, offsets) of a case appended as one batch, computed once"""
    if c not in _cache:
        r = collect(c)
        rows, offsets = r.finish()
        _cache[c] = (r, rows.cpu().numpy(), offsets)
    return _cache[c]


CASES = ["two_passes", "wave_boundary"]


@pytest.mark.parametrize("c", CASES)
def test_rows_and_offsets_equal_the_reference(c):
    g = golden()
    r, rows, offsets = one_batch(c)
    assert offsets.dtype == np.int32 and offsets.tolist() == g[c + "/offsets"].tolist()
    want = g[c + "/rows"]
    assert rows.shape == want.shape
    bad = [(i, j, rows[i, j], want[i, j]) for i, j in zip(*np.nonzero(~((rows == want) & (np.signbit(rows) == np.signbit(want)))))]
    assert bad == [], bad[:8]
    assert r.nonfinite_fields == 0 and r.unwrapped_angles is False and r.n_images == len(offsets) - 1


@pytest.mark.parametrize("c", CASES)
def test_single_image_batches_give_the_same_rows(c):
    _, rows, offsets = one_batch(c)
    rows1, offsets1 = collect(c, per_image=True).finish()
    assert offsets1.tolist() == offsets.tolist() and same(rows1.cpu().numpy(), rows)


@pytest.mark.parametrize("c", CASES)
def test_written_files_equal_the_reference_text(c, tmp_path):
    g = golden()
    r, _, _ = one_batch(c)
    ids = ["%06d" % (7 + i) for i in range(len(g[c + "/text"]))]
    texts = r.write(str(tmp_path), ids)
    assert sorted(os.listdir(str(tmp_path))) == [i + ".txt" for i in ids]
    for i, want in zip(ids, g[c + "/text"]):
        with open(os.path.join(str(tmp_path), i + ".txt"), "rb") as f:
            assert f.read() == str(want).encode()
    assert texts == [str(t) for t in g[c + "/text"]]


# ---------------------------------------------------------------------------------------------------------------------------
# the rounding
# ---------------------------------------------------------------------------------------------------------------------------
def host_round6(x):
    return np.array([float("%.6f" % v) for v in x], np.float64)


def check_round6(x):
    from groomed_nms_amd import round6
    x = np.ascontiguousarray(x, np.float64)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = round6(torch.from_numpy(x).cuda(), count=count).cpu().numpy()
    want = host_round6(x)
    bad = np.nonzero(~((got == want) & (np.signbit(got) == np.signbit(want))))[0]
    assert bad.size == 0, [(x[i].hex(), got[i], want[i]) for i in bad[:8]]
    assert int(count) == 0
    return got


def test_round6_random_magnitudes():
    rng = np.random.default_rng(20240611)
    x = rng.uniform(1.0, 10.0, 100000) * 10.0 ** rng.uniform(-9, 7, 100000) * rng.choice([-1.0, 1.0], 100000)
    assert np.abs(x).min() >= 1e-9 and np.abs(x).max() <= 1e8
    check_round6(x)


def test_round6_exact_binary_ties_go_to_even():
    k = np.arange(1, 2000, 2, dtype=np.float64)
    x = np.concatenate([k / 128.0, -k / 128.0])                          # k / 128 = ....5 at the seventh decimal, exactly
    got = check_round6(x)
    assert got[0] == 0.007812 and got[1] == 0.023438 and got[1000] == -0.007812 and got[1001] == -0.023438


def test_round6_decimal_ties_and_their_neighbours():
    rng = np.random.default_rng(7)
    k = np.concatenate([np.arange(0, 500), rng.integers(500, 10 ** 9, 500)]).astype(np.float64)
    t = (k + 0.5) / 1e6
    x = np.concatenate([t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)])
    check_round6(np.concatenate([x, -x]))


def test_round6_small_values_keep_their_sign():
    got = check_round6(np.array([1e-7, -1e-7, 0.0, -0.0, 4.9e-7, -4.9e-7, 5.1e-7, -5.1e-7, 1e-300, -1e-300]))
    assert np.signbit(got).tolist() == [False, True, False, True, False, True, False, True, False, True]
    assert got[1] == 0.0 and got[6] == 1e-6 and got[7] == -1e-6


def test_round6_passes_what_is_outside_its_contract():
    from groomed_nms_amd import round6
    x = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 1e9, 999999999.9999994, 1.5, -np.nan], np.float64)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = round6(torch.from_numpy(x).cuda(), count=count).cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[8]) and got[1:6].tolist() == x[1:6].tolist()
    assert got[6] == float("%.6f" % x[6]) and got[7] == 1.5
    assert int(count) == 7
    round6(torch.from_numpy(x).cuda(), count=count)
    assert int(count) == 14                                              # the counter accumulates
    assert round6(torch.zeros((0,), dtype=torch.float64, device="cuda")).shape == (0,)
    m = torch.from_numpy(np.array([[0.0078125, 1.0000005], [2.5e-7, -0.0234375]])).cuda()
    assert round6(m.t()).cpu().numpy().tolist() == [[0.007812, 0.0], [float("%.6f" % 1.0000005), -0.023438]]     # a strided view


# ---------------------------------------------------------------------------------------------------------------------------
# limits and the status words
# ---------------------------------------------------------------------------------------------------------------------------
CANARY = -12345.678


def test_capacity_one_below_the_need():
    c = "wave_boundary"
    g = golden()
    want = g[c + "/rows"]
    need = len(want)
    from groomed_nms_amd import KittiResults
    # the accumulator's buffers become views of larger ones: what lies behind them must stay as it is
    big = torch.full((need - 1 + 64, 14), CANARY, dtype=torch.float64, device="cuda")
    big_lbl = torch.full((need - 1 + 64,), -7, dtype=torch.int32, device="cuda")
    det, counts, p2_inv, kw = inputs(c)
    r = KittiResults(max_images=3, capacity_rows=need - 1, **kw)
    r._rows, r._lbl_index = big[:need - 1], big_lbl[:need - 1]
    r.append(det, counts, p2_inv)
    with pytest.raises(ValueError) as e:
        r.finish()
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)
    torch.cuda.synchronize()
    assert same(big[:need - 1].cpu().numpy(), want[:need - 1])           # the rows that fit are intact
    assert bool((big[need - 1:] == CANARY).all()) and bool((big_lbl[need - 1:] == -7).all())
    rows, offsets = collect(c).finish()                                  # a fresh accumulator on the same inputs
    assert same(rows.cpu().numpy(), want) and offsets.tolist() == g[c + "/offsets"].tolist()


def test_more_images_than_room():
    c = "wave_boundary"
    from groomed_nms_amd import KittiResults
    det, counts, p2_inv, kw = inputs(c)
    r = KittiResults(max_images=2, capacity_rows=200, **kw)
    meta = torch.full((r._meta.numel() + 32,), -7, dtype=torch.int32, device="cuda")
    meta[:r._meta.numel()] = 0
    r._meta = meta[:r._meta.numel()]
    r._state, r._offsets = r._meta[:16].view(torch.int64), r._meta[16:]
    r.append(det, counts, p2_inv)
    with pytest.raises(ValueError) as e:
        r.finish()
    assert "3 images" in str(e.value) and "max_images is 2" in str(e.value)
    assert meta[16:19].tolist() == golden()[c + "/offsets"].tolist()[:3] and bool((meta[19:] == -7).all())


def test_status_words_count_fields_outside_the_contract_and_bad_classes():
    from groomed_nms_amd import KittiResults, detect
    det = np.zeros((1, 5, 14), np.float32)
    det[0, :, :4] = [10, 20, 110, 90]
    det[0, :, 4] = [0.9, np.inf, 0.8, np.nan, 0.95]                      # NaN > thres is False: the row is dropped
    det[0, :, 5] = 1
    det[0, :, 6:9] = [600, 180, 20]
    det[0, :, 9:12] = [1.6, np.nan, 1e12]                                # h = NaN: h and y are not finite; l >= 1e9
    det[0, :, 12] = 0.3
    p2 = np.array([[700, 0, 600, 40], [0, 700, 180, 0], [0, 0, 1, 0.003], [0, 0, 0, 1.0]])
    p2_inv = detect.camera_constants(p2, 1.0, (1, 1), 1)[0]
    counts = torch.tensor([5], dtype=torch.int32, device="cuda")
    r = KittiResults(["Car"], 0.5, 50, 1, 10)
    r.append(torch.from_numpy(det).cuda(), counts, p2_inv)
    rows, offsets = r.finish()
    assert offsets.tolist() == [0, 4] and r.nonfinite_fields == 4 * 3 + 1 and r.unwrapped_angles is False
    rows = rows.cpu().numpy()
    assert np.isnan(rows[:, 6]).all() and np.isnan(rows[:, 10]).all() and (rows[:, 8] == float(np.float32(1e12))).all() and rows[1, 13] == np.inf
    assert rows[0, 13] == float("%.6f" % float(np.float32(0.9))) and (rows[:, 0] == 0).all()
    for cls in (0.0, 2.0, -3.0, np.nan, 3e9):                            # label index -1, 1, ... : outside the one-label table
        d = det.copy()
        d[0, 2, 5] = cls
        r = KittiResults(["Car"], 0.5, 50, 1, 10)
        r.append(torch.from_numpy(d).cuda(), counts, p2_inv)
        with pytest.raises(ValueError) as e:
            r.finish()
        assert "class index" in str(e.value)


def test_host_tensors_and_wrong_shapes_are_refused():
    from groomed_nms_amd import KittiResults, _lib
    det, counts, p2_inv, kw = inputs("wave_boundary")
    r = KittiResults(max_images=3, capacity_rows=150, **kw)
    with pytest.raises(_lib.GnmsError):
        r.append(det.cpu(), counts, p2_inv)
    for bad in ((det[..., :13], counts, p2_inv), (det.double(), counts, p2_inv), (det, counts.long(), p2_inv), (det, counts[:2], p2_inv),
                (det, counts, p2_inv.float()), (det, counts, p2_inv[:, :3])):
        with pytest.raises(ValueError):
            r.append(*bad)
    assert r.n_images == 0 and r.finish()[1].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: six images, AP through the accumulator == AP through the result files
# ---------------------------------------------------------------------------------------------------------------------------
LBLS = ["Car", "Pedestrian", "Cyclist"]
THRES, TOPN = 0.6, 40


def scene(rng, B=6, Kmax=48):
    det = np.zeros((B, Kmax, 14), np.float32)
    x1, y1 = rng.uniform(0, 1000, (B, Kmax)), rng.uniform(0, 200, (B, Kmax))
    det[..., 0], det[..., 1] = x1, y1
    det[..., 2], det[..., 3] = x1 + rng.uniform(50, 200, (B, Kmax)), y1 + rng.uniform(45, 150, (B, Kmax))
    det[..., 4] = rng.uniform(0.2, 1.0, (B, Kmax))
    det[..., 5] = rng.integers(1, 4, (B, Kmax))
    det[..., 6], det[..., 7], det[..., 8] = rng.uniform(0, 1240, (B, Kmax)), rng.uniform(120, 280, (B, Kmax)), rng.uniform(5, 60, (B, Kmax))
    det[..., 9], det[..., 10], det[..., 11] = rng.uniform(0.5, 2.0, (B, Kmax)), rng.uniform(1.3, 2.0, (B, Kmax)), rng.uniform(0.8, 4.5, (B, Kmax))
    det[..., 12] = rng.uniform(-3.1, 3.1, (B, Kmax))
    counts = np.array([Kmax, 30, 0, 41, 17, Kmax], np.int32)
    p2 = np.stack([np.array([[f, 0, 605 + b, 45.0], [0, f, 172.0, 0.2], [0, 0, 1, 0.0027], [0, 0, 0, 1]]) for b, f in enumerate(rng.uniform(705, 725, B))])
    return det, counts, p2


def test_ap_without_files_equals_ap_through_files(tmp_path):
    from groomed_nms_amd import KittiResults, detect, kitti_io, kitti_eval as K
    rng = np.random.default_rng(99)
    det, counts, p2 = scene(rng)
    B = det.shape[0]
    conf = dict(lbls=LBLS, score_thres=THRES, nms_topN_post=TOPN)
    data, labels = tmp_path / "results" / "data", tmp_path / "label_2"
    data.mkdir(parents=True)
    labels.mkdir()
    ids = ["%06d" % i for i in range(B)]
    # route B (the yardstick): the parent commit's code, image by image on the host -- and the ground truth, synthesised from its boxes
    occ = 0
    for b in range(B):
        aboxes = det[b, :counts[b]].astype(np.float64)[:TOPN]
        aboxes = aboxes[np.where(aboxes[:, 4] > THRES)[0]]
        boxes = kitti_io.convert_image_predictions_to_correct_entries(aboxes, conf, p2[b])
        kitti_io.write_image_boxes_to_txt_file(boxes, conf, str(data), ids[b])
        lines = []
        for row in boxes[::2]:                                           # every second detection has an object; the others are false positives
            jit = rng.uniform(-0.5, 0.5, 4)
            alpha = kitti_io.convertRot2Alpha(np.array([row[12]]), np.array([row[8]]), np.array([row[6]]))[0]
            vals = [alpha] + list(row[0:4] + jit) + [row[10], row[9], row[11], row[6], row[7], row[8], row[12]]
            lines.append("%s %.2f %d " % (LBLS[int(row[5]) - 1], (0.0, 0.2, 0.4)[occ % 3], occ % 3) + " ".join("%.2f" % v for v in vals))
            occ += 1
        (labels / (ids[b] + ".txt")).write_text("".join(s + "\n" for s in lines))
    variants = [K.MAIN, K.SIDE, K.DISTANCE_GRID[(30, 0.3)]]
    det_b, doff_b, names = K.load_results(str(data))
    gt, goff = K.load_labels(str(labels), names)
    via_files = K.evaluate(det_b, doff_b, gt, goff, variants=variants)
    # route A
    r = KittiResults(LBLS, THRES, TOPN, max_images=B, capacity_rows=B * TOPN)
    p2_inv = detect.camera_constants(p2, 1.0, (1, 1), B)[0]
    det_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda()
    for b0 in (0, 4):                                                    # two batches: four images, then two
        r.append(det_d[b0:b0 + 4], counts_d[b0:b0 + 4], p2_inv[b0:b0 + 4])
    rows, doff = r.finish()
    assert doff.tolist() == doff_b.tolist() and same(rows.cpu().numpy(), det_b)
    on_device = r.evaluate(gt, goff, variants=variants)
    for a, b in zip(on_device, via_files):
        assert same(a["precision"], b["precision"]) and same(a["aos"], b["aos"])
        assert a["compute_aos"] == b["compute_aos"] and a["eval_3d"].tolist() == b["eval_3d"].tolist() == [True, True, True]
    p = via_files[0]["precision"]
    assert all(p[c, m, d].max() > 0 for c in range(3) for m in range(3) for d in range(3)), "every class, metric and difficulty has matches"
    assert via_files[0]["compute_aos"] and all(via_files[0]["aos"][c, d].max() > 0 for c in range(3) for d in range(3))
    # the dictionaries of run_kitti_eval, from the accumulator instead of the folder
    got = K.evaluate_detections(r, str(labels), names, LBLS, variants=[K.MAIN, K.SIDE])
    want = [K.run_kitti_eval(str(tmp_path / "results"), str(labels), LBLS, variant=v, write=False) for v in (K.MAIN, K.SIDE)]
    assert got == want and sorted(got[0]) == sorted(k + c for k in ("det_2d_", "or_", "gr_", "det_3d_") for c in ("car", "pedestrian", "cyclist"))
    named = K.evaluate_detections(r, str(labels), names, LBLS, variants={"main": K.MAIN})
    assert named == {"main": want[0]}
