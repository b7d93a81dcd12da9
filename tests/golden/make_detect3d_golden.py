"""Generate tests/golden/detect3d.npz by IMPORTING the reference's im_detect_3d (lib/rpn_util.py:1052-1356) and calling it with a
stand-in `net` that returns prepared head tensors and an identity `preprocess`.  Runs only where the reference checkout is (first
argument, read-only); it writes data only: each case's inputs and the returned array, keyed 'case/field'.

What is stubbed, and why:
  * cv2, torchvision, easydict, shapely, visdom, lib.augmentations: imported at the top of lib/rpn_util.py, unused on this path
    (the stub modules of make_targets_golden.py);
  * Tensor.cuda / torch.cuda.FloatTensor: identity shims, the generator runs without a GPU; Tensor.masked_fill_ accepts the
    reference's uint8 mask again (torch >= 2 rejects it);
  * lib.nms.gpu_nms: the reference's compiled CUDA NMS cannot be built here.  The cases named `classic_*_hostnms` substitute THIS
    repository's host restatement, groomed_nms_amd/nms/_host.greedy_nms with the GPU kernel's rule (+1-pixel IoU in fp32, a box is
    suppressed when IoU > thresh, lib/nms/nms_kernel.cu:24-32, :71).  Those cases therefore pin the path around the NMS to the
    reference and the NMS itself to the host restatement, not to the reference's binary.

Guard band: keep decisions must not hinge on last-bit differences of exp().  A case is redrawn (new seed) until no pairwise overlap
among the NMS inputs lies within 1e-3 of nms_thres, no rescored probability lies within 1e-3 of the valid threshold, and no two
scores -- and no two valid probabilities -- are closer than 1e-6.  The number of redraws is stored per case; more than 20 is an error.

usage: python tests/golden/make_detect3d_golden.py REFERENCE_CHECKOUT"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_targets_golden import _Stub  # noqa: E402
from groomed_nms_amd import synthetic  # noqa: E402
from groomed_nms_amd.nms._host import greedy_nms, overlap_with  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(HERE, "detect3d.npz")
BAND, GAP, MAX_REDRAWS = 1e-3, 1e-6, 20


def host_gpu_nms(dets, thresh, device_id=0):
    return greedy_nms(np.asarray(dets, np.float32), thresh, shift=1, rule="le_keep", dtype=np.float32)


def load_reference():
    for name in ("cv2", "torchvision", "torchvision.transforms", "easydict", "shapely", "shapely.geometry", "visdom",
                 "lib.augmentations", "lib.nms", "lib.nms.gpu_nms"):
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules["lib.nms.gpu_nms"].gpu_nms = host_gpu_nms
    orig_fill = torch.Tensor.masked_fill_      # torch >= 2 rejects the uint8 mask of lib/groomed_nms.py:56, :73 (as in make_golden.py)
    torch.Tensor.masked_fill_ = lambda self, mask, value: orig_fill(self, mask.bool() if mask.dtype == torch.uint8 else mask, value)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor
    sys.path.insert(0, REF)
    import lib.rpn_util as rpn_util   # noqa: E402
    return rpn_util


class Conf(dict):
    __getattr__ = dict.__getitem__


# name -> (generator keywords, configuration, scale factor, (H, W) of the original image)
GRID = (4, 16, 12)          # 768 anchors
CASES = [
    ("groomed_2d", dict(), dict(use_nms_in_loss=True), 1.0),
    ("groomed_3d", dict(), dict(use_nms_in_loss=True, overlap_in_nms="3d"), 1.0),
    ("groomed_product", dict(), dict(use_nms_in_loss=True, overlap_in_nms="product"), 1.0),
    ("groomed_2d_plain_alpha", dict(decomp_alpha=False), dict(use_nms_in_loss=True, decomp_alpha=False), 1.0),
    ("groomed_2d_acceptance", dict(), dict(use_nms_in_loss=True, predict_acceptance_prob=True, use_acceptance_prob_for_nms=True), 1.0),
    ("groomed_2d_clip_scale", dict(), dict(use_nms_in_loss=True, clip_boxes=True), 0.5),
    ("groomed_3d_scale", dict(), dict(use_nms_in_loss=True, overlap_in_nms="3d", diff_nms_temperature=0.01), 1.5),
    ("groomed_product_acceptance_scale", dict(), dict(use_nms_in_loss=True, overlap_in_nms="product", predict_acceptance_prob=True,
                                                      use_acceptance_prob_for_nms=True, clip_boxes=True), 0.75),
    ("groomed_2d_few_anchors", dict(A_grid=(2, 12, 12)), dict(use_nms_in_loss=True), 1.0),
    ("groomed_2d_all_low", dict(score_hi=0.25), dict(use_nms_in_loss=True), 1.0),
    ("classic_hostnms", dict(), dict(), 1.0),
    ("classic_clip_scale_hostnms", dict(), dict(clip_boxes=True, predict_acceptance_prob=True, use_acceptance_prob_for_nms=True), 0.5),
    ("classic_topn_plain_alpha_hostnms", dict(decomp_alpha=False), dict(decomp_alpha=False, nms_topN_pre=600), 1.0),
    ("groomed_3d_topn", dict(), dict(use_nms_in_loss=True, overlap_in_nms="3d", nms_topN_pre=300), 1.0),      # 768 -> 300 (below the 500 of :1293)
]


def run_case(rpn_util, seed, gen_kw, conf_kw, scale):
    rng = np.random.default_rng(seed)
    kw = dict(A_grid=GRID)
    kw.update(gen_kw)
    d = synthetic.detection_heads(rng, 1, **kw)
    conf = Conf(anchors=d["anchors"], bbox_means=d["bbox_means"], bbox_stds=d["bbox_stds"], nms_thres=0.4, nms_topN_pre=3000, clip_boxes=False,
                decomp_alpha=True)
    conf.update(conf_kw)
    hs = 96                                                        # the image the stand-in net sees: [1, 3, hs, ws]
    h_orig = int(round(hs / scale))
    assert h_orig * scale == hs
    im = np.zeros((h_orig, 600, 3), np.float32)

    def preprocess(x):
        return np.zeros((3, hs, 8), np.float32)

    def net(x):
        t = torch.from_numpy
        return (None, t(d["prob"].copy()), t(d["bbox_2d"].copy()), t(d["bbox_3d"].copy()), None, t(d["rois"].copy()), t(d["acceptance"].copy()), None)
    seen = {}
    real_nms, real_gpu = rpn_util.differentiable_nms, rpn_util.gpu_nms

    def spy_nms(scores_unsorted, iou_unsorted, **k):
        out = real_nms(scores_unsorted=scores_unsorted, iou_unsorted=iou_unsorted, **k)
        seen.update(scores=np.asarray(scores_unsorted), iou=np.asarray(iou_unsorted), prob=out[2].numpy(), thr=k["valid_box_prob_threshold"])
        return out

    def spy_gpu(dets, thresh, device_id=0):
        seen.update(scores=dets[:, 4], iou=np.stack([overlap_with(dets[i, :4], dets[:, :4], 1, np.float32) for i in range(len(dets))]))
        return real_gpu(dets, thresh, device_id=device_id)
    rpn_util.differentiable_nms, rpn_util.gpu_nms = spy_nms, spy_gpu
    try:
        out = rpn_util.im_detect_3d(im, net, conf, preprocess, d["p2"])
    finally:
        rpn_util.differentiable_nms, rpn_util.gpu_nms = real_nms, real_gpu
    # the guard band
    ok = True
    iou = seen["iou"][np.triu_indices(len(seen["iou"]), 1)]
    ok &= not np.any(np.abs(iou - conf.nms_thres) < BAND)
    s = np.sort(seen["scores"].astype(np.float64))
    ok &= not np.any(np.diff(s) < GAP)
    allscores = np.amax(d["prob"][0, :, 1:], 1)
    if conf.get("use_acceptance_prob_for_nms"):
        allscores = allscores * d["acceptance"][0, :, 0]
    ok &= not np.any(np.diff(np.sort(allscores.astype(np.float64))) < GAP)
    if "prob" in seen:
        p = seen["prob"].astype(np.float64)
        ok &= not np.any(np.abs(p - seen["thr"]) < BAND)
        ok &= not np.any(np.diff(np.sort(p[p > seen["thr"]])) < GAP)
    return ok, d, conf, im.shape[:2], scale, out


def main():
    if not REF:
        sys.exit(__doc__)
    rpn_util = load_reference()
    z = {}
    for ci, (name, gen_kw, conf_kw, scale) in enumerate(CASES):
        for redraw in range(MAX_REDRAWS + 1):
            ok, d, conf, hw, scale, out = run_case(rpn_util, 5000 + 100 * ci + redraw, gen_kw, conf_kw, scale)
            if ok:
                break
        else:
            sys.exit("case %s needs more than %d redraws" % (name, MAX_REDRAWS))
        p = name + "/"
        for k in ("prob", "bbox_2d", "bbox_3d", "rois", "anchors", "bbox_means", "bbox_stds", "p2"):
            z[p + k] = d[k]
        if conf.get("use_acceptance_prob_for_nms"):                # (stored where it is read: the file stays small)
            z[p + "acceptance"] = d["acceptance"]
        z[p + "im_hw"] = np.array(hw, np.int64)
        z[p + "scale_factor"] = np.array(scale)
        z[p + "redraws"] = np.array(redraw)
        for k in ("use_nms_in_loss", "overlap_in_nms", "decomp_alpha", "predict_acceptance_prob", "use_acceptance_prob_for_nms", "clip_boxes",
                  "nms_thres", "nms_topN_pre", "diff_nms_temperature"):
            if k in conf:
                z[p + "conf_" + k] = np.array(conf[k])
        z[p + "aboxes"] = out
        print("%-36s A=%5d redraws=%d kept=%d" % (name, d["rois"].shape[0], redraw, len(out)))
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
