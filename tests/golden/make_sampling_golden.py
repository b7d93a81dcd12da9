"""Generate tests/golden/sampling.npz by RUNNING the reference's RPN_3D_loss.forward (lib/loss/rpn_3d.py) on the CPU.  Runs only where
the reference checkout (abhi1kumar/groomed_nms) is; it writes data only: per shape the shared inputs (cls, prob), per case the
configuration, the label column that the reference's compute_targets returned for each image (recorded by wrapping it, so the
sampler tests do not depend on the targets kernel), and the reference's loss, stats (fg, bg, cls) and cls.grad after loss.backward().

Only the classification term is switched on (cls_2d_lambda = 1, iou_2d_lambda = bbox_2d_lambda = bbox_3d_lambda = 0, decomp_alpha,
no NMS in the loss, no acceptance prob), so cls.grad is non-zero exactly on the sampled anchors and proportional to their weights.
The reference's module-level imports that the loss never uses (cv2, torchvision, shapely, visdom, lib.augmentations, the compiled
lib.nms.gpu_nms, plot.common_operations, easydict) are stubbed, and its .cuda() calls / torch.cuda tensor types are mapped to the CPU.

np.argsort's order among equal keys is not defined, so every stored case is checked to have no equal keys across either cut.
usage: python tests/golden/make_sampling_golden.py REFERENCE_CHECKOUT"""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sampling.npz")
LBLS = ["Car", "Pedestrian", "Cyclist"]
ILBLS = ["Van", "Truck", "Person_sitting", "Tram", "Misc", "DontCare"]


class _Stub(types.ModuleType):
    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return object


class EasyDict(dict):
    def __init__(self, d=None, **kw):
        super().__init__(dict(d or {}, **kw))

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)

    __setattr__ = dict.__setitem__


def load_reference():
    for name in ("cv2", "torchvision", "torchvision.transforms", "easydict", "shapely", "shapely.geometry", "visdom",
                 "lib.augmentations", "lib.nms", "lib.nms.gpu_nms", "plot", "plot.common_operations"):
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.modules["lib.nms.gpu_nms"].gpu_nms = None
    sys.modules["plot.common_operations"].__all__ = []
    sys.modules["lib.augmentations"].__all__ = []
    sys.modules["easydict"].EasyDict = EasyDict
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.LongTensor = torch.LongTensor
    torch.cuda.FloatTensor = torch.FloatTensor
    torch.cuda.BoolTensor = torch.BoolTensor
    torch.cuda.ByteTensor = torch.ByteTensor
    sys.path.insert(0, REF)
    import lib.loss.rpn_3d as L   # noqa: E402
    return L


def anchor_grid(rng, H, W, A, stride=16):
    wh = np.stack([rng.uniform(16, 90, A), rng.uniform(16, 70, A)], 1)
    a2 = np.concatenate([-wh / 2, wh / 2], 1)
    ys, xs = np.meshgrid(np.arange(H) * stride, np.arange(W) * stride, indexing="ij")
    shifts = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], 1).astype(np.float64)
    rois = (shifts[:, None, :] + a2[None]).reshape(-1, 4)
    tracker = np.tile(np.arange(A), H * W).astype(np.float64)
    anchors = np.zeros((A, 11))
    anchors[:, :4] = a2
    anchors[:, 4] = rng.uniform(5, 40, A)
    anchors[:, 5:8] = rng.uniform(0.5, 4, (A, 3))
    anchors[:, 8] = rng.uniform(-3, 3, A)
    anchors[:, 9] = np.sin(anchors[:, 8])
    anchors[:, 10] = np.cos(anchors[:, 8])
    return np.concatenate([rois, tracker[:, None]], 1).astype(np.float32), anchors


def make_gts(rng, rois, n, kind):
    """kind: 'valid' (classes of LBLS), 'ignored' (every GT carries ign), 'none' (no GT at all)"""
    gts = []
    if kind == "none":
        return gts
    n_all = n + (2 if kind == "valid" else 0)                     # a valid scene also carries two ignored GTs (ignore anchors)
    pick = rng.choice(len(rois), n_all, replace=False)
    for j, i in enumerate(pick):
        b = rois[i, :4].astype(np.float64) + rng.normal(0, 4.0, 4)
        b[2:] = np.maximum(b[2:], b[:2] + 6)
        b3 = np.zeros(16)
        b3[0:2] = (b[:2] + b[2:]) / 2
        b3[2] = rng.uniform(5, 50)
        b3[3:6] = rng.uniform(0.5, 4, 3)
        b3[6:] = rng.uniform(-3, 3, 10)
        b3[14:16] = rng.integers(0, 2, 2)
        gts.append(EasyDict(cls=LBLS[rng.integers(0, 3)], ign=(kind == "ignored" or j >= n), visibility=1.0,
                            bbox_full=np.array([b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]), bbox_3d=b3))
    return gts


def conf_of(anchors, box_samples, fg_fraction, focal_loss):
    return EasyDict(lbls=LBLS, ilbls=ILBLS, anchors=anchors, bbox_means=np.zeros((1, 13)), bbox_stds=np.ones((1, 13)), feat_stride=16,
                    fg_fraction=fg_fraction, box_samples=box_samples, ign_thresh=0.5, nms_thres=0.4, fg_thresh=0.5, bg_thresh_lo=0.0,
                    bg_thresh_hi=0.5, best_thresh=0.35, hard_negatives=True, focal_loss=focal_loss, crop_size=[512, 1760],
                    cls_2d_lambda=1, iou_2d_lambda=0, bbox_2d_lambda=0, bbox_3d_lambda=0, min_gt_vis=0.65, min_gt_h=0, max_gt_h=1e9,
                    decomp_alpha=True, use_nms_in_loss=False, predict_acceptance_prob=False)


def cut_keys_distinct(col, prob, box_samples, fg_fraction):
    """True when, for each class the quota cuts, the keys on the two sides of the cut differ (and no key there is NaN)"""
    R = len(col)
    fg, bg = np.flatnonzero(col > 0), np.flatnonzero(col < 0)
    if np.isinf(box_samples):
        return True
    fg_num = min(round(R * box_samples * fg_fraction), len(fg))
    bg_num = min(round(R * box_samples - fg_num), len(bg))
    for idx, num, lab in ((fg, fg_num, col[fg].astype(int)), (bg, bg_num, np.zeros(len(bg), int))):
        if num > 0 and num != len(idx):
            k = np.sort(prob[idx, lab])
            if not k[num - 1] < k[num]:
                return False
    return True


def main():
    if not REF:
        sys.exit(__doc__)
    L = load_reference()
    z = {}
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    inf = float("inf")
    for shape, (H, W, A) in (("r210", (5, 7, 6)), ("r1332", (3, 37, 12))):
        rng = np.random.default_rng(20260 + H * W * A)
        rois, anchors = anchor_grid(rng, H, W, A)
        R = len(rois)
        assert R == H * W * A
        B, C = 2, 4
        r3 = np.zeros((R, 11), np.float32)
        r3[:, :4] = rois[:, :4]
        r3[:, 4:] = anchors[rois[:, 4].astype(np.int64), 4:] + rng.normal(0, 0.05, (R, 7))
        cen = ((rois[:, :2] + rois[:, 2:4]) / 2).astype(np.float32)
        n_gt = 5 if R < 1000 else 14
        scenes = {"valid": [make_gts(rng, rois, n_gt, "valid"), make_gts(rng, rois, n_gt, "valid")]}
        scenes["no_gt"] = [scenes["valid"][0], make_gts(rng, rois, 0, "none")]
        scenes["all_ign"] = [make_gts(rng, rois, n_gt, "ignored"), scenes["valid"][1]]
        cls = torch.from_numpy(rng.normal(0, 1.5, (B, R, C)).astype(np.float32))
        prob = torch.softmax(cls, dim=2)
        bbox_2d = torch.from_numpy(rng.normal(0, 0.2, (B, R, 4)).astype(np.float32))
        bbox_3d = torch.from_numpy(rng.normal(0, 0.2, (B, R, 11)).astype(np.float32))
        z[shape + "/cls"] = cls.numpy()
        z[shape + "/prob"] = prob.numpy()

        # name: scene, box_samples, fg_fraction, focal_loss, the regime the case is there for (fg cut, bg cut) per processed image
        cases = [("both_cut", "valid", 0.25, 0.04, 0, (True, True)),
                 ("both_cut_focal2", "valid", 0.25, 0.04, 2, (True, True)),
                 ("neither", "valid", 1.0, 0.5, 0, (False, False)),
                 ("neither_focal2", "valid", 1.0, 0.5, 2, (False, False)),
                 ("bg_cut", "valid", 0.5, 0.5, 0, (False, True)),
                 ("quota_zero", "valid", 0.0003, 0.2, 0, (False, False)),
                 ("inf", "valid", inf, 0.2, 0, (False, False)),
                 ("inf_no_fraction", "valid", inf, None, 0, (False, False)),
                 ("inf_no_fraction_focal2", "valid", inf, None, 2, (False, False)),
                 ("no_gt_image", "no_gt", 0.25, 0.04, 0, (True, True)),
                 ("all_ignored_image", "all_ign", 0.25, 0.04, 2, (True, True))]
        for name, scene, bs, ff, focal, regime in cases:
            imobjs = [EasyDict(gts=g, p2=p2.copy(), scale_factor=1.0) for g in scenes[scene]]
            cols = {}
            real = L.compute_targets
            state = {"calls": 0}

            def recording(gts_val, gts_ign, box_lbls, rois_np, *a, **k):
                t, o, g = real(gts_val, gts_ign, box_lbls, rois_np, *a, **k)
                cols[state["order"][state["calls"]]] = t[:, 4].copy()
                state["calls"] += 1
                return t, o, g
            # the images the loop does not skip (:406), in order
            state["order"] = [b for b in range(B) if any((not g.ign) for g in scenes[scene][b])]
            L.compute_targets = recording
            try:
                loss_mod = L.RPN_3D_loss(conf_of(anchors, bs, ff, focal), verbose=True)
                x = cls.clone().requires_grad_(True)
                loss, stats = loss_mod(x, prob, bbox_2d, bbox_3d, imobjs, [H, W], rois=torch.from_numpy(rois)[None].repeat(B, 1, 1),
                                       rois_3d=torch.from_numpy(r3)[None].repeat(B, 1, 1),
                                       rois_3d_cen=torch.from_numpy(cen)[None].repeat(B, 1, 1))
                loss.backward()
            finally:
                L.compute_targets = real
            assert state["calls"] == len(state["order"])
            col = np.zeros((B, R), np.float32)
            val_counts = np.zeros(B, np.int32)
            for b in range(B):
                if b in cols:
                    col[b] = cols[b]
                    val_counts[b] = sum(1 for g in scenes[scene][b] if not g.ign)
                    n_fg, n_bg = int((col[b] > 0).sum()), int((col[b] < 0).sum())
                    assert n_fg > 0 and n_bg > 0 and (col[b] == 0).any(), (shape, name, b, n_fg, n_bg)
                    if not np.isinf(bs):
                        fg_num = min(round(R * bs * ff), n_fg)
                        bg_num = min(round(R * bs - fg_num), n_bg)
                        got = (fg_num > 0 and fg_num != n_fg, bg_num > 0 and bg_num != n_bg)
                        assert got == regime, (shape, name, b, n_fg, n_bg, fg_num, bg_num)
                        if name == "quota_zero":
                            assert fg_num == 0 and bg_num == 0
                    assert cut_keys_distinct(col[b], prob[b].numpy(), bs, ff), "%s/%s image %d ties at a cut: use another seed" % (shape, name, b)
            st = {s["name"]: float(s["val"]) for s in stats}
            p = "%s/%s/" % (shape, name)
            z[p + "config"] = np.array([bs, np.nan if ff is None else ff, focal], np.float64)      # fg_fraction NaN = None
            z[p + "target_labels"] = col
            z[p + "val_counts"] = val_counts
            z[p + "loss"] = np.array(loss.detach().numpy(), np.float32)
            z[p + "stats"] = np.array([st.get("fg", np.nan), st.get("bg", np.nan), st.get("cls", np.nan)], np.float64)
            z[p + "grad"] = x.grad.numpy().copy()
            print(p, "loss %.6f" % float(loss.detach()), "fg %s bg %s" % (st.get("fg"), st.get("bg")),
                  "sampled rows", int((x.grad.numpy() != 0).any(axis=2).sum()),
                  [(int((col[b] > 0).sum()), int((col[b] < 0).sum())) for b in range(B)])
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
