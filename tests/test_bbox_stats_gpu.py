"""compute_bbox_stats on the GPU (csrc/bbox_stats.hip) against the reference's own run (tests/golden/bbox_stats.npz):
per-image foreground counts and float32 sums bit for bit, the means within the reference's float128 accumulation error, the deviations
within 2^-40, bitwise independence of batch size, visit order and run, and a loss module built from the prepared conf."""
import numpy as np
import pytest
import torch

import test_bbox_stats_host as H
from groomed_nms_amd import dataset_stats as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return H.golden()


@pytest.fixture(scope="module")
def prepared(z):
    """conf after the two calls, the way scripts/train_rpn_3d.py:76-79 makes them; computed once and left unchanged"""
    conf = H.conf_of(z)
    imdb = H.imdb_of(z)
    D.generate_anchors(conf, imdb, None)
    D.compute_bbox_stats(conf, imdb, None)
    return conf, imdb


@pytest.mark.parametrize("name,use_trunc", [("mean", True), ("dev", False)])
def test_per_image_counts_and_float32_sums_bit_for_bit(z, name, use_trunc):
    conf = H.conf_of(z, anchors=z["anchors"])
    p = D.image_partials(conf, H.imdb_of(z), use_trunc, batch_size=4)
    assert np.array_equal(p.used, z["imdb/n_gts"] > 0)
    print(name, "foreground counts", p.counts.tolist(), "golden", z[name + "/fg_counts"].tolist())
    assert np.array_equal(p.counts, z[name + "/fg_counts"].astype(np.int32))
    assert p.sums.dtype == np.float32 and p.sums.shape == (len(p.used), 13)
    assert np.array_equal(H.bits(p.sums), H.bits(z[name + "/sums"]))


def test_deviation_partials_equal_a_float64_restatement(z, prepared):
    conf, imdb = prepared
    means = conf.bbox_means[0]
    p = D.image_partials(conf, imdb, False, means=means, batch_size=3)
    assert np.array_equal(p.counts, z["dev/fg_counts"].astype(np.int32))
    ends = np.cumsum(z["dev/fg_counts"])
    for i, (c, e) in enumerate(zip(z["dev/fg_counts"], ends)):
        want = np.zeros(13)
        for row in z["dev/rows"][e - c:e].astype(np.float64):          # in anchor order, one subtraction, one product, one addition
            d = row - means
            want = want + d * d
        assert np.array_equal(H.bits(p.sq_sums[i]), H.bits(want)), i


def test_means_within_the_reference_accumulation_error(z, prepared):
    conf, _ = prepared
    got, ref = conf.bbox_means, z["bbox_means"]
    assert got.shape == (1, 13) and got.dtype == np.float64
    N = len(z["imdb/n_gts"])
    n = int(z["mean/fg_counts"].sum())
    s = np.abs(z["mean/sums"].astype(np.float64)).sum(axis=0)
    # the reference's own error: one rounding to float128's 64-bit mantissa per image added; then the rounding to float64
    bound = N * 2.0 ** -63 * s / n + 2.0 ** -52 * np.abs(ref[0])
    err = np.abs(got[0] - ref[0])
    print("means |got - ref|", err.tolist(), "bound", bound.tolist())
    assert np.all(err <= bound)


def test_deviations_within_2_to_the_minus_40(z, prepared):
    conf, _ = prepared
    got, ref = conf.bbox_stds, z["bbox_stds"]
    assert got.shape == (1, 13) and got.dtype == np.float64
    assert z["dev/fg_counts"].max() < 2 ** 13 and z["mean/fg_counts"].max() < 2 ** 13
    rel = np.abs(got[0] / ref[0] - 1.0)
    print("stds |got / ref - 1|", rel.tolist())
    assert np.all(rel <= 2.0 ** -40)


def test_results_do_not_depend_on_batch_size_visit_order_or_run(z, prepared):
    conf, imdb = prepared
    rng = np.random.default_rng(3)
    runs = [dict(batch_size=1), dict(batch_size=4), dict(batch_size=None), dict(batch_size=2, visit_order=rng.permutation(len(imdb)).tolist()),
            dict(batch_size=D.DEFAULT_BATCH)]
    for kw in runs:
        c = H.conf_of(z, anchors=z["anchors"])
        D.compute_bbox_stats(c, imdb, None, **kw)
        assert np.array_equal(H.bits(c.bbox_means), H.bits(conf.bbox_means)), kw
        assert np.array_equal(H.bits(c.bbox_stds), H.bits(conf.bbox_stds)), kw
    order = rng.permutation(len(imdb)).tolist()
    a = D.image_partials(conf, imdb, True, batch_size=1)
    b = D.image_partials(conf, imdb, True, batch_size=None, visit_order=order)
    assert np.array_equal(H.bits(a.sums), H.bits(b.sums)) and np.array_equal(a.counts, b.counts)


def test_an_imdb_without_foreground_gives_the_reference_zeros(z):
    imdb = H.imdb_of(z)
    conf = H.conf_of(z, anchors=z["anchors"])
    D.compute_bbox_stats(conf, [imdb[6], imdb[3]], None)
    for got, key in ((conf.bbox_means, "nofg/bbox_means"), (conf.bbox_stds, "nofg/bbox_stds")):
        assert got.shape == (1, 13) and np.array_equal(H.bits(got), H.bits(z[key]))


def test_cache_folder_is_written_and_read_back(z, prepared, tmp_path):
    conf, imdb = prepared
    c = H.conf_of(z, anchors=z["anchors"])
    D.compute_bbox_stats(c, imdb, str(tmp_path))
    assert (tmp_path / "bbox_means.pkl").exists() and (tmp_path / "bbox_stds.pkl").exists()
    again = H.conf_of(z, anchors=z["anchors"])
    D.compute_bbox_stats(again, None, str(tmp_path))                    # read: the imdb is not touched
    assert np.array_equal(H.bits(again.bbox_means), H.bits(conf.bbox_means)) and np.array_equal(H.bits(again.bbox_stds), H.bits(conf.bbox_stds))


def test_partials_entry_validates_its_arguments():
    from groomed_nms_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.zeros((1, 8, 23), dtype=torch.float32, device=dev)
    ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    sums = torch.zeros((1, 13), dtype=torch.float32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    call = lambda B, R, ld, n, s, c: lib.gnms_bbox_stats_partials(t.data_ptr(), B, R, ld, ids.data_ptr(), n, None, s, None, c, None)   # noqa: E731
    assert call(1, 8, 13, 1, sums.data_ptr(), cnt.data_ptr()) == -1     # ld < 14
    assert call(2, 8, 23, 1, sums.data_ptr(), cnt.data_ptr()) == -1     # more images in the batch than in the data set
    assert call(1, 8, 23, 1, None, cnt.data_ptr()) == -1                # the mean pass without sums
    assert call(-1, 8, 23, 1, sums.data_ptr(), cnt.data_ptr()) == -1
    assert call(0, 8, 23, 1, sums.data_ptr(), cnt.data_ptr()) == 0
    # an id outside the data set writes nothing
    ids.fill_(5)
    sums.fill_(7.0)
    assert call(1, 8, 23, 1, sums.data_ptr(), cnt.data_ptr()) == 0
    torch.cuda.synchronize()
    assert float(sums.min()) == 7.0


def test_the_prepared_conf_constructs_the_loss_and_one_forward_runs(z, prepared):
    from groomed_nms_amd import loss, heads
    conf, imdb = prepared
    full = H.AttrDict(conf)
    full.update(fg_fraction=0.2, box_samples=64, nms_thres=0.4, hard_negatives=True, focal_loss=0, cls_2d_lambda=1, iou_2d_lambda=1,
                bbox_2d_lambda=0, bbox_3d_lambda=1, use_nms_in_loss=False)
    module = loss.RPN_3D_loss(full, verbose=False, capacity=16)
    dev = torch.device("cuda", torch.cuda.current_device())
    images = [imdb[1], imdb[4]]                                          # one feat_size, (6, 22)
    p2 = np.array([[700.0, 0, 600.0, 40.0], [0, 700.0, 180.0, 2.0], [0, 0, 1.0, 0.003]])
    imobjs = [H.AttrDict(gts=im.gts, p2=p2, scale_factor=im.scale * conf.test_scale / im.imH) for im in images]
    feat_size = (6, 22)
    A, C = conf.anchors.shape[0], len(conf.lbls) + 1
    R = A * feat_size[0] * feat_size[1]
    g = torch.Generator(device="cpu").manual_seed(11)
    cls = torch.randn((2, R, C), generator=g).to(dev).requires_grad_(True)
    prob = torch.softmax(cls, dim=2)
    bbox_2d = (0.1 * torch.randn((2, R, 4), generator=g)).to(dev).requires_grad_(True)
    bbox_3d = (0.1 * torch.randn((2, R, 10), generator=g)).to(dev).requires_grad_(True)
    assert heads.anchor_grid(conf.anchors, feat_size, conf.feat_stride)[0].shape[0] == R
    total, stats = module(cls, prob, bbox_2d, bbox_3d, imobjs, feat_size)
    assert total.dim() == 0 and bool(torch.isfinite(total))
    assert any(s["name"] == "total" for s in stats)
