"""Generate tests/golden/heads.npz by RUNNING the reference's own RPN.forward (models/densenet121_3d_dilate_decomp_alpha.py) on the CPU.
Runs only where the reference checkout (abhi1kumar/groomed_nms) is; it writes data only.

The RPN object is made without its __init__ (no DenseNet, no torchvision): base and prop_feats are identities and the fifteen head
modules are channel slices of the input, so the input IS the stacked maps and everything behind the convolutions (:166-245) runs as
the reference wrote it.  The reference is loaded through make_sampling_golden.load_reference(), which stubs the modules that are not
installed and maps .cuda() / torch.cuda tensor types to the CPU.

Per shape (B, A, H, W, C): the fifteen maps, five random cotangents, the anchors and the stride, the reference's rois, rois_3d and
rois_2d_cen; per case: the reference's cls, prob, bbox_2d, bbox_3d, acceptance and torch.autograd.grad's gradients of the maps.  Cases:
every shape with all heads and all five cotangents, one without the acceptance head and one whose only cotangent is bbox_3d's (both on
the maps of the second shape).  Maps and cotangents are multiples of 1/64, which keeps the file small; logits include rows with
entries of +-100 and rows with all-equal entries.
usage: python tests/golden/make_heads_golden.py REFERENCE_CHECKOUT"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_sampling_golden as S   # noqa: E402

OUT = os.path.join(HERE, "heads.npz")
SHAPES = [(1, 1, 1, 1, 2), (2, 3, 5, 7, 4), (2, 36, 2, 9, 4), (1, 2, 3, 130, 3)]
STRIDE = 16


class Slice(nn.Module):
    def __init__(self, lo, hi):
        super().__init__()
        self.lo, self.hi = lo, hi

    def forward(self, x):
        return x[:, self.lo:self.hi]


def make_rpn(M, A, C, anchors, with_acceptance):
    net = M.RPN.__new__(M.RPN)
    nn.Module.__init__(net)
    net.base = nn.Identity()
    net.prop_feats = nn.Identity()
    net.cls = Slice(0, C * A)
    at = C * A
    for name in ("x", "y", "w", "h", "x3d", "y3d", "z3d", "w3d", "h3d", "l3d", "alpha", "axis", "head"):
        setattr(net, "bbox_" + name, Slice(at, at + A))
        at += A
    net.acceptance_prob = Slice(at, at + A)
    net.softmax = nn.Softmax(dim=1)
    net.sigmoid = nn.Sigmoid()
    net.num_classes, net.num_anchors, net.anchors, net.feat_stride, net.feat_size = C, A, anchors, STRIDE, [0, 0]
    net.predict_acceptance_prob, net.acceptance_prob_mode = with_acceptance, "regress"
    net.train()
    return net


def sixty_fourths(rng, scale, shape):
    return (np.round(rng.normal(0, scale, shape) * 64) / 64).astype(np.float32)


def run(M, maps, A, C, anchors, with_acceptance, cot_names, cots):
    leaves = [torch.from_numpy(m.copy()).requires_grad_(True) for m in maps]
    net = make_rpn(M, A, C, anchors, with_acceptance)
    cls, prob, b2, b3, feat_size, rois, rois_3d, cen, acc, acc_cls = net(torch.cat(leaves, dim=1))
    assert acc_cls is None and (acc is not None) == with_acceptance
    outs = dict(cls=cls, prob=prob, bbox_2d=b2, bbox_3d=b3, acceptance=acc)
    used = leaves if with_acceptance else leaves[:14]
    grads = torch.autograd.grad([outs[n] for n in cot_names], used, [torch.from_numpy(cots[n]) for n in cot_names], allow_unused=True)
    grads = [np.zeros(tuple(l.shape), np.float32) if g is None else g.numpy() for g, l in zip(grads, used)]
    tables = dict(rois=rois[0].numpy(), rois_3d=rois_3d[0].numpy(), rois_2d_cen=cen[0].numpy())
    assert tables["rois"].dtype == np.float32 and tables["rois_3d"].dtype == np.float32
    return {k: v.detach().numpy() for k, v in outs.items() if v is not None}, grads, tables


def main():
    if not S.REF:
        sys.exit(__doc__)
    S.load_reference()
    tv = sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))     # not installed; RPN.forward never touches it
    if not isinstance(getattr(tv, "models", None), types.ModuleType):
        tv.models = sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
    M = importlib.import_module("models.densenet121_3d_dilate_decomp_alpha")
    import test_heads_host as T
    z = {}
    for B, A, H, W, C in SHAPES:
        shape = "s_%d_%d_%d_%d_%d" % (B, A, H, W, C)
        rng = np.random.default_rng(31 * H * W * A + C)
        R = A * H * W
        wh = np.stack([rng.uniform(16, 90, A), rng.uniform(16, 70, A)], 1)
        anchors = np.zeros((A, 11))
        anchors[:, :4] = np.concatenate([-wh / 2, wh / 2], 1)
        anchors[:, 4] = rng.uniform(5, 40, A)
        anchors[:, 5:8] = rng.uniform(0.5, 4, (A, 3))
        anchors[:, 8] = rng.uniform(-3, 3, A)
        anchors[:, 9], anchors[:, 10] = np.sin(anchors[:, 8]), np.cos(anchors[:, 8])
        logits = sixty_fourths(rng, 2.0, (B, C, R))
        if R > 8:                                                       # rows with +-100 entries, rows with all-equal entries
            rows = rng.choice(R, min(R, 24), replace=False)
            for i, r in enumerate(rows):
                b = i % B
                if i % 3 == 0:
                    logits[b, :, r] = logits[b, 0, r]
                elif i % 3 == 1:
                    logits[b, rng.integers(0, C), r] = 100.0
                    logits[b, rng.integers(0, C), r] = -100.0
                else:
                    logits[b, :, r] = rng.choice([-100.0, 100.0], C)
        maps = [logits.reshape(B, C * A, H, W)] + [sixty_fourths(rng, 1.5, (B, A, H, W)) for _ in range(14)]
        for k in (12, 13, 14):                                           # the sigmoids' far ends
            flat = maps[k].reshape(-1)
            if flat.size > 8:
                flat[rng.choice(flat.size, 4, replace=False)] = [-100.0, 100.0, -20.0, 20.0]
        cots = dict(cls=sixty_fourths(rng, 1.0, (B, R, C)), prob=sixty_fourths(rng, 1.0, (B, R, C)), bbox_2d=sixty_fourths(rng, 1.0, (B, R, 4)),
                    bbox_3d=sixty_fourths(rng, 1.0, (B, R, 10)), acceptance=sixty_fourths(rng, 1.0, (B, R, 1)))
        for n, m in zip(T.MAP_NAMES, maps):
            z["%s/map_%s" % (shape, n)] = m
        for n, g in cots.items():
            z["%s/g_%s" % (shape, n)] = g
        z[shape + "/anchors"] = anchors
        z[shape + "/feat_stride"] = np.array(STRIDE, np.float64)
        for case, (of_shape, has_acc, which) in T.CASES.items():
            if of_shape != shape:
                continue
            outs, grads, tables = run(M, maps, A, C, anchors, has_acc, which, cots)
            for k, v in outs.items():
                assert np.all(np.isfinite(v)), (case, k)
                z["%s/%s" % (case, k)] = v
            for n, g in zip(T.MAP_NAMES, grads):
                assert np.all(np.isfinite(g)) and g.dtype == np.float32, (case, n)
                z["%s/d_%s" % (case, n)] = g
            if case == shape:
                for k, v in tables.items():
                    z["%s/%s" % (shape, k)] = v
            print(case, {k: v.shape for k, v in outs.items()})
    np.savez_compressed(OUT, **z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d keys, %d bytes)" % (OUT, len(z), size))
    assert size < 1 << 20
    from conftest import Golden
    e = T.reference_errors(Golden("heads.npz"))
    print("e_ref:", e)
    assert all(v > 0 for v in e.values()), e


if __name__ == "__main__":
    main()
