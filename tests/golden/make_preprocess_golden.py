"""Generate tests/golden/preprocess.npz by IMPORTING the reference's lib/augmentations.py and running its own Augmentation, Preprocess,
RandomMirror.flip_gts and Resize.scale_gts (through Augmentation.__call__, i.e. through the reference's Compose) on small synthetic
images and imobjs built here.  Runs only where the reference checkout is (the first argument, read-only); it writes data only: the
uint8 images, the conf values, the reference's float32 outputs, the imobjs before and after, the mirror draws and NumPy's global
generator state after the run.

cv2 is not installed where this was generated.  The stub's `resize` asserts that the requested size IS the image's size and returns a
copy, so the goldens cover a SCALE FACTOR OF 1 ONLY: mirror, crop, pad, normalisation, channel order and the whole imobj side, but not
the resample (tests/test_preprocess_gpu.py holds that to a float64 restatement instead).  torchvision, easydict, shapely, visdom and,
where missing, matplotlib and PIL are stubbed as well; none of them is used on this path (distort_prob = -1).
usage: python tests/golden/make_preprocess_golden.py REFERENCE_CHECKOUT"""
import copy
import importlib
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess.npz")
SEED = 5                                               # mirrors every source at least once and leaves it at least once (asserted below)
CROP = [32, 96]
SOURCES = ((32, 80), (32, 96), (32, 120))              # pad, exact fit, crop
CALLS = 9                                              # Augmentation calls, the sources in turn
GT_KEYS = ("gts", "gts_1")
EGO_KEYS = ("ego_10", "ego_32")


class _Stub(types.ModuleType):
    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return object


class Obj(dict):
    """what easydict gives the reference: keys as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__

    def __deepcopy__(self, memo):
        return Obj({k: copy.deepcopy(v, memo) for k, v in self.items()})


def load_reference():
    names = ["cv2", "torchvision", "torchvision.transforms", "easydict", "shapely", "shapely.geometry", "visdom"]
    for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "matplotlib.backends", "matplotlib.backends.backend_agg",
                 "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:                                                                 # noqa: BLE001
            names.append(name)
    for name in names:
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules.pop("lib.augmentations", None)        # another generator's stub of the module under test

    def resize(image, wh):
        assert (image.shape[1], image.shape[0]) == tuple(int(v) for v in wh), "the stubbed cv2.resize only stands in for a scale factor of 1"
        return image.copy()
    sys.modules["cv2"].resize = resize
    sys.path.insert(0, REF)
    import lib.augmentations as A   # noqa: E402
    return A


def make_conf():
    return Obj(image_means=[0.485, 0.456, 0.406], image_stds=[0.229, 0.224, 0.225], crop_size=list(CROP), mirror_prob=0.5, distort_prob=-1)


def make_gt(rng, H, W, p2, ry, with_vis):
    w, h = rng.uniform(6, 30), rng.uniform(6, 20)
    x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
    b3 = np.zeros(16)
    b3[0:2] = (x + w / 2 + rng.normal(0, 1), y + h / 2 + rng.normal(0, 1))                # projected centre
    b3[2] = rng.uniform(5, 40)                                                            # depth
    b3[3:6] = rng.uniform(0.5, 4.5, 3)
    b3[10] = ry
    c3 = np.linalg.inv(p2).dot(np.array([b3[0] * b3[2], b3[1] * b3[2], b3[2], 1]))
    b3[7:10] = c3[:3]
    b3[6] = ry - np.arctan2(-c3[2], c3[0]) - 0.5 * np.pi
    b3[11] = rng.uniform(-0.2, 0.2)
    b3[12:16] = rng.normal(0, 1, 4)
    gt = Obj(cls="Car", bbox_full=np.array([x, y, w, h]), bbox_3d=b3, center_3d=c3[:3].copy())
    if with_vis:
        gt.bbox_vis = np.array([x + 1, y + 1, w * 0.8, h * 0.9])
    return gt


def make_imobj(rng, H, W):
    p2 = np.array([[60.0, 0, W / 2 - 0.3, 4.1], [0, 60.0, H / 2 + 0.2, -0.6], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    rys = [-3.1, -0.3, 0.4, 3.12, -np.pi, rng.uniform(-3, 3), rng.uniform(-3, 3)]
    imobj = Obj(p2=p2, p2_inv=np.linalg.inv(p2), imH=H, imW=W,
                ego_10=[0.3, -0.02, 1.1, 0.01, -3.2, 0.5], ego_32=[-0.4, 0.0, 0.9, -0.02, 0.2, 3.3])
    imobj.gts = [make_gt(rng, H, W, p2, ry, True) for ry in rys]
    imobj.gts_1 = [make_gt(rng, H, W, p2, ry, False) for ry in (rng.uniform(-3, 3), 1.5)]
    return imobj


def imobj_arrays(imobj, prefix, z):
    for key in GT_KEYS:
        gts = imobj[key]
        z["%s/%s/bbox_full" % (prefix, key)] = np.array([g.bbox_full for g in gts], np.float64)
        z["%s/%s/bbox_3d" % (prefix, key)] = np.array([g.bbox_3d for g in gts], np.float64)
        z["%s/%s/center_3d" % (prefix, key)] = np.array([g.center_3d for g in gts], np.float64)
        if all("bbox_vis" in g for g in gts):
            z["%s/%s/bbox_vis" % (prefix, key)] = np.array([g.bbox_vis for g in gts], np.float64)
    for key in EGO_KEYS:
        z["%s/%s" % (prefix, key)] = np.array(imobj[key], np.float64)
    z[prefix + "/p2_inv"] = np.array(imobj.p2_inv, np.float64)
    if "scale_factor" in imobj:
        z[prefix + "/scale_factor"] = np.array(imobj.scale_factor, np.float64)


def main():
    if not REF:
        sys.exit(__doc__)
    A = load_reference()
    rng = np.random.default_rng(2028)
    conf = make_conf()
    z = {"seed": np.array(SEED), "crop_size": np.array(CROP), "calls": np.array(CALLS)}
    for k in ("image_means", "image_stds", "mirror_prob", "distort_prob"):
        z["conf/" + k] = np.array(conf[k])
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SOURCES]
    imobjs = [make_imobj(rng, H, W) for H, W in SOURCES]
    for i, im in enumerate(images):
        z["image/%d" % i] = im

    # Preprocess, as lib/rpn_util.py:1074 and scripts/test_rpn_3d.py:78 call it
    pre = A.Preprocess(conf.crop_size, conf.image_means, conf.image_stds)
    for i, im in enumerate(images):
        out = pre(im)
        assert out.dtype == np.float32 and out.shape == (3, CROP[0], CROP[1]), (out.dtype, out.shape)
        z["preprocess/%d" % i] = np.ascontiguousarray(out)

    # Augmentation, as lib/imdb_util.py:511 calls it, CALLS times under one seed; the draws are recorded on the way through
    draws = []
    rand = np.random.rand

    def recording_rand(*a):
        draws.append(rand(*a))
        return draws[-1]
    aug = A.Augmentation(conf)
    np.random.seed(SEED)
    np.random.rand = recording_rand
    try:
        for k in range(CALLS):
            i = k % len(images)
            imobj = copy.deepcopy(imobjs[i])
            imobj_arrays(imobj, "in/%d" % k, z)
            out, imobj2 = aug(images[i], imobj)
            assert imobj2 is imobj and out.dtype == np.float32 and out.shape == (CROP[0], CROP[1], 3), (out.dtype, out.shape)
            z["augment/%d" % k] = np.ascontiguousarray(out)                               # HWC, still BGR: the swap follows at imdb_util.py:522-526
            imobj_arrays(imobj, "out/%d" % k, z)
    finally:
        np.random.rand = rand
    state = np.random.get_state()
    assert state[0] == "MT19937"
    z["state/keys"], z["state/pos"] = np.array(state[1], np.uint32), np.array(state[2])
    assert len(draws) == CALLS, "one draw per image with distort_prob <= 0"
    z["draws"] = np.array(draws, np.float64)
    mirrored = z["draws"] <= conf.mirror_prob
    z["mirrored"] = mirrored
    for i in range(len(images)):                                                          # every source both ways
        ks = [k for k in range(CALLS) if k % len(images) == i]
        assert any(mirrored[k] for k in ks) and not all(mirrored[k] for k in ks), (i, mirrored.tolist())
    # the ground truths exercise what the issue lists
    ry_in = np.concatenate([z["in/%d/gts/bbox_3d" % k][:, 10] for k in range(CALLS) if mirrored[k]])
    assert (ry_in < 0).any() and (ry_in > 0).any() and (np.abs(np.abs(ry_in) - np.pi) < 0.05).any() and (ry_in == -np.pi).any()
    axis = np.concatenate([z["out/%d/gts/bbox_3d" % k][:, 14] for k in range(CALLS) if mirrored[k]])
    head = np.concatenate([z["out/%d/gts/bbox_3d" % k][:, 15] for k in range(CALLS) if mirrored[k]])
    assert set(axis.tolist()) == {0.0, 1.0} and set(head.tolist()) == {0.0, 1.0}, (axis, head)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes); mirrored %s" % (OUT, len(z), os.path.getsize(OUT), mirrored.astype(int).tolist()))


if __name__ == "__main__":
    main()
