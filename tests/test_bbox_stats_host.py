"""dataset_stats without a GPU: generate_anchors against the reference bit for bit, the NumPy restatement of the
per-image float32 sums, the record packing with its host-side scaling, the grouping by feat_size, the cache folder, the refusals.
The golden (tests/golden/bbox_stats.npz, written by make_bbox_stats_golden.py) is the reference's own generate_anchors and
compute_bbox_stats on a ten-image imdb with three feat_sizes."""
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN

from groomed_nms_amd import dataset_stats as D

COLUMNS = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13)


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class Attr:
    """a ground truth or image with attribute access only"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


_Z = None


def golden():
    global _Z
    if _Z is None:
        z = np.load(os.path.join(GOLDEN, "bbox_stats.npz"))
        _Z = {k: z[k] for k in z.keys()}
    return _Z


def conf_of(z, **over):
    conf = AttrDict()
    for k, v in z.items():
        if k.startswith("conf/"):
            conf[k[5:]] = v.tolist()
    conf.update(over)
    return conf


def imdb_of(z, attr=False):
    """the stored imdb as objects: dicts with key access, or (attr) plain objects with attribute access"""
    make = (lambda **kw: Attr(**kw)) if attr else (lambda **kw: AttrDict(**kw))
    imdb, at = [], 0
    for i, n in enumerate(z["imdb/n_gts"]):
        gts = []
        for j in range(at, at + int(n)):
            gts.append(make(cls=str(z["imdb/cls"][j]), ign=bool(z["imdb/ign"][j]), visibility=float(z["imdb/visibility"][j]),
                            trunc=float(z["imdb/trunc"][j]), bbox_full=z["imdb/bbox_full"][j].copy(), bbox_3d=z["imdb/bbox_3d"][j].copy()))
        at += int(n)
        imdb.append(make(gts=gts, scale=float(z["imdb/scale"][i]), imH=int(z["imdb/imH"][i]), imW=int(z["imdb/imW"][i])))
    return imdb


def ragged(z, name, field, width=None):
    """per image the rows of a flat stored array"""
    counts = z["%s/%s_counts" % (name, field)] if field != "fg" else z[name + "/fg_counts"]
    flat = z["%s/%s" % (name, field)]
    ends = np.cumsum(counts)
    return [flat[e - c:e] for c, e in zip(counts, ends)]


def restate_filter(rec, n, min_gt_vis, min_gt_h, use_trunc):
    """gnms_gt_filter at scale 1 and max_gt_h = inf, in NumPy: (gts_val, gts_ign, gts_3d, box_lbls) of one image's records"""
    val, ign_rows, g3, lbl = [], [], [], []
    for row in rec[:n]:
        ign = row[21] != 0 or row[22] < min_gt_vis or row[3] < min_gt_h or row[20] == 0
        if use_trunc:
            ign = ign or row[23] > max(1.0 - min_gt_vis, 0.0)
        if row[20] < 0:
            continue
        box = [row[0], row[1], row[2] + (row[0] - 1.0), row[3] + (row[1] - 1.0)]
        if ign:
            ign_rows.append(box)
        else:
            val.append(box)
            g3.append(row[4:20])
            lbl.append(int(row[20]))
    return (np.array(val, np.float64).reshape(-1, 4), np.array(ign_rows, np.float64).reshape(-1, 4), np.array(g3, np.float64).reshape(-1, 16),
            np.array(lbl, np.int64))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ the fixture is what the issue asks for
def test_the_fixture_covers_the_cases():
    z = golden()
    assert z["anchors"].shape[0] < 12 and z["gts_per_candidate_anchor"].min() == 0 and np.sort(z["gts_per_candidate_anchor"])[1] >= 2
    assert (z["imdb/n_gts"] == 0).sum() >= 1
    with_gts = z["imdb/n_gts"] > 0
    assert np.any(with_gts & (z["mean/gts_val_counts"] == 0) & (z["dev/gts_val_counts"] == 0))          # all ignored or removed
    assert len({tuple(f) for f in z["mean/feat_size"][with_gts]}) >= 2
    assert np.any(z["imdb/scale"] != 1.0)
    assert np.any(z["mean/fg_counts"] != z["dev/fg_counts"])                                             # use_trunc bites
    assert z["dev/fg_counts"].max() < 2 ** 13


# ------------------------------------------------------------------------------------------------ generate_anchors
@pytest.mark.parametrize("attr", [False, True])
def test_generate_anchors_equals_the_reference_bit_for_bit(attr):
    z = golden()
    conf = conf_of(z)
    D.generate_anchors(conf, imdb_of(z, attr=attr), None)
    assert conf.anchors.dtype == np.float64 and conf.anchors.shape == z["anchors"].shape == (11, 11)
    assert np.array_equal(bits(conf.anchors), bits(z["anchors"]))
    assert conf["anchors"] is conf.anchors


# ------------------------------------------------------------------------------------------------ NumPy's order
def test_sequential_float32_sum_equals_the_stored_sums():
    z = golden()
    for name in ("mean", "dev"):
        rows = z[name + "/rows"]
        ends = np.cumsum(z[name + "/fg_counts"])
        for i, (c, e) in enumerate(zip(z[name + "/fg_counts"], ends)):
            got = D.sequential_f32_sum(rows[e - c:e])
            assert got.dtype == np.float32
            assert np.array_equal(bits(got), bits(z[name + "/sums"][i])), (name, i)


def test_sequential_float32_sum_equals_numpy_axis0_on_random_rows():
    rng = np.random.default_rng(7)
    for m in (1, 2, 7, 8, 9, 127, 128, 129, 1000, 4097):
        t = (rng.normal(0, 1, (m + 50, 23)) * rng.choice([1e-3, 1.0, 50.0], (1, 23))).astype(np.float32)
        inds = np.sort(rng.choice(m + 50, m, replace=False))
        for sl in (slice(0, 4), slice(5, 14)):
            ref = np.sum(t[inds, sl], axis=0)                          # lib/rpn_util.py:642-643
            assert ref.dtype == np.float32
            assert np.array_equal(bits(D.sequential_f32_sum(t[inds, sl])), bits(ref)), m
    assert not np.signbit(D.sequential_f32_sum(np.full((2, 3), -0.0, np.float32))).any()
    assert not np.signbit(np.sum(np.full((2, 3), -0.0, np.float32), axis=0)).any()


# ------------------------------------------------------------------------------------------------ packing, grouping
@pytest.mark.parametrize("attr", [False, True])
def test_pack_records_scales_on_the_host_as_the_reference_does(attr):
    z = golden()
    conf = conf_of(z, anchors=z["anchors"])
    p = D.pack_records(conf, imdb_of(z, attr=attr))
    N = len(z["imdb/n_gts"])
    assert p.records.shape == (N, int(z["imdb/n_gts"].max()), 24) and p.records.dtype == np.float64
    assert np.array_equal(p.counts, z["imdb/n_gts"].astype(np.int32))
    with_gts = z["imdb/n_gts"] > 0
    assert np.array_equal(p.feat_sizes[with_gts], z["mean/feat_size"][with_gts])
    for name, use_trunc in (("mean", True), ("dev", False)):
        val, ign, g3 = ragged(z, name, "gts_val"), ragged(z, name, "gts_ign"), ragged(z, name, "gts_3d")
        lbl_ends = np.cumsum(z[name + "/gts_val_counts"])
        for i in range(N):
            got = restate_filter(p.records[i], p.counts[i], conf.min_gt_vis, conf.min_gt_h, use_trunc)
            assert np.array_equal(bits(got[0]), bits(val[i])), (name, i)
            assert np.array_equal(bits(got[1]), bits(ign[i])), (name, i)
            assert np.array_equal(bits(got[2]), bits(g3[i])), (name, i)
            assert np.array_equal(got[3], z[name + "/box_lbls"][lbl_ends[i] - len(val[i]):lbl_ends[i]]), (name, i)
        assert np.all(p.records[np.arange(p.records.shape[1])[None, :] >= p.counts[:, None]] == 0)


def test_group_by_feat_size():
    z = golden()
    conf = conf_of(z, anchors=z["anchors"])
    p = D.pack_records(conf, imdb_of(z))
    groups = D.group_by_feat_size(p)
    assert list(groups) == [(6, 20), (6, 22), (8, 25)]
    assert groups[(6, 20)] == [0, 6, 9] and groups[(6, 22)] == [1, 4, 7] and groups[(8, 25)] == [2, 5, 8]      # image 3 has no gts
    order = [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    shuffled = D.group_by_feat_size(p, order)
    assert list(shuffled) == [(6, 20), (8, 25), (6, 22)] and shuffled[(6, 20)] == [9, 6, 0]
    assert {k: sorted(v) for k, v in shuffled.items()} == {k: sorted(v) for k, v in groups.items()}


# ------------------------------------------------------------------------------------------------ the cache folder
def test_cache_folder_round_trip_without_a_gpu(tmp_path):
    z = golden()
    conf = conf_of(z)
    folder = str(tmp_path)
    D.generate_anchors(conf, imdb_of(z), folder)
    with open(os.path.join(folder, "anchors.pkl"), "rb") as f:
        stored = pickle.load(f)                                         # a plain pickle of the ndarray, lib/util.py:233-248
    assert isinstance(stored, np.ndarray) and np.array_equal(bits(stored), bits(z["anchors"]))
    again = conf_of(z)
    D.generate_anchors(again, None, folder)                             # read back: the imdb is not touched
    assert np.array_equal(bits(again.anchors), bits(z["anchors"]))
    # a set written by plain pickle, as the reference's pickle_write does
    for name, key in (("bbox_means.pkl", "bbox_means"), ("bbox_stds.pkl", "bbox_stds")):
        with open(os.path.join(folder, name), "wb") as f:
            pickle.dump(z[key], f)
    D.compute_bbox_stats(again, None, folder)
    assert np.array_equal(bits(again.bbox_means), bits(z["bbox_means"])) and np.array_equal(bits(again.bbox_stds), bits(z["bbox_stds"]))
    assert again.bbox_means.shape == (1, 13) and again.bbox_means.dtype == np.float64


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("key,value", [("has_3d", False), ("decomp_alpha", False), ("cluster_anchors", 1), ("has_vel", True)])
@pytest.mark.parametrize("fn", ["generate_anchors", "compute_bbox_stats"])
def test_unsupported_keys_raise_naming_the_key(fn, key, value):
    z = golden()
    conf = conf_of(z, anchors=z["anchors"])
    conf[key] = value
    with pytest.raises(NotImplementedError, match=key):
        getattr(D, fn)(conf, imdb_of(z), None)


def test_absent_optional_keys_are_fine_and_absent_required_ones_are_not():
    z = golden()
    conf = conf_of(z)
    assert "cluster_anchors" not in conf and "has_vel" not in conf
    D.generate_anchors(conf, imdb_of(z), None)
    del conf["decomp_alpha"]
    with pytest.raises(NotImplementedError, match="decomp_alpha"):
        D.generate_anchors(conf, imdb_of(z), None)


@pytest.mark.parametrize("fn", ["generate_anchors", "pack_records"])
def test_more_than_256_ground_truths_raise(fn):
    z = golden()
    conf = conf_of(z, anchors=z["anchors"])
    imdb = imdb_of(z)
    imdb[0].gts = [imdb[0].gts[0]] * 257
    with pytest.raises(ValueError, match="257"):
        getattr(D, fn)(conf, imdb) if fn == "pack_records" else D.generate_anchors(conf, imdb, None)


def test_the_reference_without_foreground_gives_zeros():
    """the reference divides 0 by 1e-10 (:579, :652, :721): means and deviations are +0; the GPU test holds the device to it"""
    z = golden()
    for k in ("nofg/bbox_means", "nofg/bbox_stds"):
        assert z[k].shape == (1, 13) and z[k].dtype == np.float64 and not z[k].any() and not np.signbit(z[k]).any()
