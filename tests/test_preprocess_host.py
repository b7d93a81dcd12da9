"""The image front end without a GPU: a NumPy restatement of the whole front end (mirror, bilinear resample, crop / pad,
normalise; `restate`, shared with tests/test_preprocess_gpu.py) against the reference's own Augmentation and Preprocess
(tests/golden/preprocess.npz, written by make_preprocess_golden.py: scale factor 1 only), the host side of preprocess.Augmentation --
the draws, flip_gts, ego_mirror, scale_gts -- against the reference's imobjs bit for bit, the descriptor table, and the refusals."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from groomed_nms_amd import preprocess as P

GT_KEYS = ("gts", "gts_1")
EGO_KEYS = ("ego_10", "ego_32")
GT_FIELDS = ("bbox_full", "bbox_vis", "bbox_3d", "center_3d")


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


_Z = None


def golden():
    global _Z
    if _Z is None:
        z = np.load(os.path.join(GOLDEN, "preprocess.npz"))
        _Z = {k: z[k] for k in z.keys()}
    return _Z


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def conf_of(z, **over):
    conf = AttrDict(crop_size=z["crop_size"].tolist())
    for k, v in z.items():
        if k.startswith("conf/"):
            conf[k[5:]] = v.tolist()
    conf.update(over)
    return conf


def sources(z):
    return [z["image/%d" % i] for i in range(3)]


def call_images(z):
    """the image of each of the golden's Augmentation calls"""
    src = sources(z)
    return [src[k % len(src)] for k in range(int(z["calls"]))]


def imobj_of(z, k, prefix="in"):
    """the stored imobj of call k, as the dict-like object the reference gets from easydict"""
    imobj = AttrDict(p2_inv=z["%s/%d/p2_inv" % (prefix, k)].copy())
    for key in EGO_KEYS:
        imobj[key] = z["%s/%d/%s" % (prefix, k, key)].tolist()
    for key in GT_KEYS:
        n = len(z["%s/%d/%s/bbox_full" % (prefix, k, key)])
        gts = []
        for j in range(n):
            gt = AttrDict(cls="Car")
            for f in GT_FIELDS:
                name = "%s/%d/%s/%s" % (prefix, k, key, f)
                if name in z:
                    gt[f] = z[name][j].copy()
            gts.append(gt)
        imobj[key] = gts
    return imobj


def assert_imobj_equals(imobj, z, k):
    for key in GT_KEYS:
        for f in GT_FIELDS:
            name = "out/%d/%s/%s" % (k, key, f)
            if name in z:
                got = np.array([gt[f] for gt in imobj[key]], np.float64)
                assert np.array_equal(bits(got), bits(z[name])), name
            else:
                assert all(f not in gt for gt in imobj[key]), name
    for key in EGO_KEYS:
        assert np.array_equal(bits(np.array(imobj[key], np.float64)), bits(z["out/%d/%s" % (k, key)])), (k, key)
    assert np.array_equal(bits(np.array(imobj["scale_factor"], np.float64)), bits(z["out/%d/scale_factor" % k]))


# ------------------------------------------------------------------------------------------------ the restatement
def taps(n_dst, n_src):
    """source taps of n_dst output positions over n_src samples: (d + 0.5) * (n_src / n_dst) - 0.5 in float64, rounded to float32;
    floor and fraction; both taps clamped to the edge.  The weights 1 - f and f are float32 VALUES (rounded once, as the kernel's)."""
    d = np.arange(n_dst, dtype=np.float64)
    s = ((d + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(np.float32)
    fl = np.floor(s)
    f = (s - fl).astype(np.float32)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n_src - 1), np.clip(i + 1, 0, n_src - 1), (np.float32(1) - f).astype(np.float32), f


def restate(img, size, means, stds, mirror=False, dtype=np.float64, w=None):
    """The front end of one uint8 [H, W, 3] BGR image -> [h, W_out, 3], still BGR (as Augmentation returns it), with every operation
    after the float32-rounded coefficients done in `dtype`: float64 is the yardstick of the resample, float32 is the kernel's own
    arithmetic (one IEEE rounding per operation, NumPy's and the kernel's alike) and the reference's at a scale factor of 1.
    w: a width after the resize other than Resize's own (a descriptor table may hold any)."""
    H, W, _ = img.shape
    scale_factor = size[0] / H
    h = int(np.round(H * scale_factor))
    w = int(np.round(W * scale_factor)) if w is None else w
    src = (img[:, ::-1, :] if mirror else img).astype(dtype)                              # RandomMirror comes before Resize
    x0, x1, wx0, wx1 = taps(w, W)
    y0, y1, wy0, wy1 = taps(h, H)
    hor = src[:, x0, :] * wx0.astype(dtype)[None, :, None] + src[:, x1, :] * wx1.astype(dtype)[None, :, None]
    ver = hor[y0] * wy0.astype(dtype)[:, None, None] + hor[y1] * wy1.astype(dtype)[:, None, None]
    if len(size) > 1:
        if w > size[1]:
            ver = ver[:, :size[1], :]
        elif w < size[1]:
            ver = np.pad(ver, [(0, 0), (0, size[1] - w), (0, 0)], "constant")
    out = ver / dtype(255.0)
    out = out - np.array(means, np.float32).astype(dtype)
    out = out / np.array(stds, np.float32).astype(dtype)
    assert out.dtype == dtype
    return out


def to_planes(hwc):
    """the swap and transpose of lib/imdb_util.py:522-526 and Preprocess.__call__: [h, w, 3] BGR -> [3, h, w] RGB"""
    return np.ascontiguousarray(np.transpose(hwc[:, :, (2, 1, 0)], [2, 0, 1]))


# ------------------------------------------------------------------------------------------------ against the goldens
def test_golden_is_what_the_issue_asks_for():
    z = golden()
    assert z["crop_size"].tolist() == [32, 96]
    assert [im.shape for im in sources(z)] == [(32, 80, 3), (32, 96, 3), (32, 120, 3)]
    assert z["mirrored"].any() and not z["mirrored"].all()


@pytest.mark.parametrize("i", range(3))
def test_restated_preprocess_is_the_reference_bit_for_bit(i):
    z = golden()
    conf = conf_of(z)
    got = to_planes(restate(sources(z)[i], conf.crop_size, conf.image_means, conf.image_stds, dtype=np.float32))
    want = z["preprocess/%d" % i]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want))


def test_restated_augmentation_is_the_reference_bit_for_bit():
    z = golden()
    conf = conf_of(z)
    for k, img in enumerate(call_images(z)):
        got = restate(img, conf.crop_size, conf.image_means, conf.image_stds, mirror=bool(z["mirrored"][k]), dtype=np.float32)
        assert np.array_equal(bits(got), bits(z["augment/%d" % k])), k
    # the padding is normalised, not zero, and a mirrored image is not its original
    pad = z["augment/0"][:, 80:, :]
    want = ((np.float32(0) / np.float32(255) - np.array(conf.image_means, np.float32)) / np.array(conf.image_stds, np.float32)).astype(np.float32)
    assert np.array_equal(bits(pad), bits(np.broadcast_to(want, pad.shape)))
    assert not np.array_equal(z["augment/0"], z["augment/3"]) and bool(z["mirrored"][0]) != bool(z["mirrored"][3])


@pytest.mark.parametrize("batches", [(9,), (3, 3, 3), (1, 4, 2, 2)])
def test_host_pass_draws_and_imobjs_are_the_reference_bit_for_bit(batches):
    z = golden()
    aug = P.Augmentation(conf_of(z))
    images = call_images(z)
    imobjs = [imobj_of(z, k) for k in range(len(images))]
    saved = np.random.get_state()
    try:
        np.random.seed(int(z["seed"]))
        flags, at = [], 0
        for n in batches:
            flags += aug.host_pass([im.shape for im in images[at:at + n]], imobjs[at:at + n])
            at += n
        state = np.random.get_state()
    finally:
        np.random.set_state(saved)
    assert flags == z["mirrored"].tolist()
    # as many values drawn as the reference drew: the generator stands where the reference left it
    assert state[0] == "MT19937" and int(state[2]) == int(z["state/pos"]) and np.array_equal(state[1], z["state/keys"])
    for k, imobj in enumerate(imobjs):
        assert_imobj_equals(imobj, z, k)


def test_flip_uses_the_width_before_the_resize_and_none_imobjs_still_draw():
    aug = P.Augmentation(AttrDict(image_means=[0.5] * 3, image_stds=[0.25] * 3, crop_size=[64, 96], mirror_prob=1.0, distort_prob=-1))
    gt = AttrDict(bbox_full=np.array([3.0, 4.0, 10.0, 8.0]))
    imobj = AttrDict(gts=[gt])
    saved = np.random.get_state()
    try:
        np.random.seed(0)
        flags = aug.host_pass([(32, 50, 3), (32, 50, 3)], [imobj, None])
        after = np.random.get_state()
        np.random.seed(0)
        np.random.rand(2)
        assert np.array_equal(after[1], np.random.get_state()[1]) and after[2] == np.random.get_state()[2]
    finally:
        np.random.set_state(saved)
    assert flags == [True, True] and imobj.scale_factor == 2.0
    assert gt.bbox_full.tolist() == [(50 - 3.0 - 10.0) * 2, 8.0, 20.0, 16.0]


# ------------------------------------------------------------------------------------------------ table and refusals
def test_describe_lays_the_images_out_and_rounds_half_to_even():
    table, nbytes, H_out, W_out = P.describe([(375, 1242, 3), (370, 1224, 3)], [512, 1760], mirror=[False, True])
    assert table.dtype == np.int64 and table.shape == (2, P.DESC) and (H_out, W_out) == (512, 1760)
    assert table[0].tolist() == [0, 375, 1242, int(np.round(1242 * (512 / 375))), 0]
    assert table[1, 0] % 256 == 0 and table[1, 0] >= 375 * 1242 * 3 and table[1, 4] == 1
    assert nbytes >= table[1, 0] + 370 * 1224 * 3 and nbytes % 256 == 0
    assert P.resized_width(4, 3, 6) == (1.5, 4)                                           # np.round(4.5): half to even
    assert P.resized_width(4, 5, 6) == (1.5, 8)                                           # np.round(7.5)
    assert P.describe([(4, 3, 3)], [6])[2:] == (6, 4)                                     # a one-element size: the width is the image's
    assert P.describe([], [6, 8])[1:] == (0, 6, 8)


def test_argument_errors():
    img = np.zeros((8, 8, 3), np.uint8)
    m, s = [0.5] * 3, [0.25] * 3
    with pytest.raises(ValueError):
        P.describe([(8, 8, 3)], [8, 8, 8])
    with pytest.raises(ValueError):
        P.describe([(8, 8, 3)], [7.5, 8])
    with pytest.raises(ValueError):
        P.describe([(8, 8, 3), (8, 8, 3)], [8, 8], mirror=[True])
    with pytest.raises(ValueError):
        P.describe([(8, 8)], [8, 8])
    with pytest.raises(ValueError):
        P.describe([(8, 8, 3), (8, 9, 3)], [16])                                          # one-element size, two widths
    with pytest.raises(ValueError):
        P.preprocess_images([img], [8, 8], [0.5] * 2, s)
    with pytest.raises(TypeError):
        P.preprocess_images([img.astype(np.float32)], [8, 8], m, s)
    with pytest.raises(TypeError):
        P.preprocess_images([[1, 2, 3]], [8, 8], m, s)
    with pytest.raises(ValueError):
        P.Preprocess([8, 8], [0.5] * 4, s)
    aug = P.Augmentation(AttrDict(image_means=m, image_stds=s, crop_size=[8, 8], mirror_prob=0.5, distort_prob=-1))
    with pytest.raises(ValueError):
        aug.host_pass([(8, 8, 3)], [None, None])


def test_not_implemented_branches():
    m, s = [0.5] * 3, [0.25] * 3
    with pytest.raises(NotImplementedError, match="distort_prob"):
        P.Augmentation(AttrDict(image_means=m, image_stds=s, crop_size=[8, 8], mirror_prob=0.5, distort_prob=0.5))
    with pytest.raises(NotImplementedError, match="channels"):
        P.preprocess_images([np.zeros((8, 8, 6), np.uint8)], [8, 8], m, s)                # the video inputs
    with pytest.raises(NotImplementedError, match="scale factor"):
        P.preprocess_images([np.zeros((16, 8, 3), np.uint8)], [8, 8], m, s)               # a reduction
    aug = P.Augmentation(AttrDict(image_means=m, image_stds=s, crop_size=[8, 8], mirror_prob=0.5, distort_prob=-1))
    saved = np.random.get_state()
    with pytest.raises(NotImplementedError, match="channels"):                            # refused before a value is drawn
        aug([np.zeros((8, 8, 1), np.uint8)], [None])
    assert np.array_equal(saved[1], np.random.get_state()[1]) and saved[2] == np.random.get_state()[2]
