"""Generate tests/golden/iou_grad.npz by IMPORTING the reference's lib/core.py and lib/groomed_nms.py and letting torch autograd
differentiate them in float32 on the CPU.  Runs only where the reference checkout is (the first argument, read-only); it writes data only.

  iou/<tag>/{a, b, cotangent, grad_a, grad_b}     lib.core.iou(a, b).backward(cotangent); rectangular, self (b absent: iou(a, a)) and ties
  layer/<tag>/{boxes, scores, weights, boxes_grad, kw/...}
        differentiable_nms(scores, iou(boxes, boxes), **kw)[2] with boxes.requires_grad, N = 60, loss = sum(weights * prob):
        default, group cap 5, unmasked groups, ungrouped, sigmoidal pruning

The inputs come from the builders of tests/test_iou_grad_host.py (seeded NumPy), so the file regenerates bit for bit.  Conditions on
the reference, asserted here: no IoU within 8 eps of nms_threshold; no rescored probability within 8 eps of the valid-box threshold or of
a clamp bound (exact 0 and 1 apart: saturated values and boxes in no group); no two distinct boxes share a coordinate, except in the
case that is there for the ties.

lib/core.py imports easydict, shapely, matplotlib and cv2 at module top; none is used here, so those that are missing are stubbed.
torch >= 2 rejects the uint8 mask of lib/groomed_nms.py:56/:73: masked_fill_ is shimmed out of tree, as in make_golden.py.
usage: python tests/golden/make_iou_grad_golden.py REFERENCE_CHECKOUT"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "iou_grad.npz")
EPS = float(np.finfo(np.float32).eps)
N_LAYER = 60

LAYER_CASES = {
    "default": dict(),
    "cap5": dict(group_size=5),
    "unmasked": dict(mask_group_boxes=False),
    "ungrouped": dict(group_boxes=False),
    "sigmoidal": dict(pruning_method="sigmoidal", temperature=0.1),
}
DEFAULTS = dict(nms_threshold=0.4, valid_box_prob_threshold=0.3)


class _Stub(types.ModuleType):
    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return object


def load_reference():
    orig = torch.Tensor.masked_fill_

    def masked_fill_compat(self, mask, value):
        return orig(self, mask.bool() if mask.dtype == torch.uint8 else mask, value)

    torch.Tensor.masked_fill_ = masked_fill_compat
    for name in ("easydict", "shapely", "shapely.geometry", "matplotlib", "matplotlib.pyplot", "cv2", "visdom", "torchvision",
                 "torchvision.transforms", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:                                                                 # noqa: BLE001
            if name not in sys.modules:
                sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    import lib.core as core           # noqa: E402
    spec = importlib.util.spec_from_file_location("ref_groomed_nms", os.path.join(REF, "lib", "groomed_nms.py"))
    gn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gn)
    return core, gn


def distinct_coordinates(*box_sets):
    allb = np.concatenate(box_sets, 0)
    for c in (0, 1):                                                   # x coordinates among themselves, y among themselves
        v = np.concatenate([allb[:, c], allb[:, c + 2]])
        if len(np.unique(v)) != len(v):
            return False
    return True


def iou_record(core, out, tag, a, b, g):
    ta = torch.tensor(a, requires_grad=True)
    if b is None:
        core.iou(ta, ta).backward(torch.tensor(g))
    else:
        tb = torch.tensor(b, requires_grad=True)
        core.iou(ta, tb).backward(torch.tensor(g))
        out["iou/%s/b" % tag] = b
        out["iou/%s/grad_b" % tag] = tb.grad.numpy().copy()
    out["iou/%s/a" % tag] = a
    out["iou/%s/cotangent" % tag] = g
    out["iou/%s/grad_a" % tag] = ta.grad.numpy().copy()


def layer_record(core, gn, out, tag, kw, T):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(6000 + sorted(LAYER_CASES).index(tag))
    boxes = synthetic.clustered_boxes_2d(rng, N_LAYER, 10)
    scores = synthetic.tie_free_scores(rng, N_LAYER)
    weights = rng.uniform(-1, 2, size=N_LAYER).astype(np.float32)
    assert distinct_coordinates(boxes), tag
    k = dict(DEFAULTS)
    k.update(kw)
    tb = torch.tensor(boxes, requires_grad=True)
    m = core.iou(tb, tb)
    assert float((m.detach() - k["nms_threshold"]).abs().min()) > 8 * EPS, "%s: an IoU sits within 8 eps of nms_threshold" % tag
    # the clamp's output before the valid-box threshold is applied: a second run with that threshold at 0
    probe = gn.differentiable_nms(torch.tensor(scores), m.detach(), **dict(k, valid_box_prob_threshold=0.0))[2].numpy()
    inside = probe[(probe != 0.0) & (probe != 1.0)]
    for bound in (0.0, 1.0, k["valid_box_prob_threshold"]):
        assert not len(inside) or float(np.abs(inside - bound).min()) > 8 * EPS, "%s: a rescored probability sits within 8 eps of %g" % (tag, bound)
    prob = gn.differentiable_nms(torch.tensor(scores), m, **k)[2]
    (prob * torch.tensor(weights)).sum().backward()
    assert tb.grad is not None and bool(torch.isfinite(tb.grad).all()) and bool(tb.grad.any()), tag
    out["layer/%s/boxes" % tag] = boxes
    out["layer/%s/scores" % tag] = scores
    out["layer/%s/weights" % tag] = weights
    out["layer/%s/prob" % tag] = prob.detach().numpy().copy()
    out["layer/%s/boxes_grad" % tag] = tb.grad.numpy().copy()
    for key, v in kw.items():
        out["layer/%s/kw/%s" % (tag, key)] = np.array(v)


def main():
    assert REF and os.path.isdir(REF), __doc__
    torch.manual_seed(0)
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.dirname(HERE))                          # tests/: the case builders
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))         # the repository: groomed_nms_amd.synthetic
    import test_iou_grad_host as T
    core, gn = load_reference()
    out = {}
    a, b = T.clustered_pair(101, 37, 53)
    assert distinct_coordinates(a, b)
    iou_record(core, out, "rect_37x53", a, b, T.cotangent(1, 37, 53))
    a, b = T.clustered_pair(102, 64, 65)
    assert distinct_coordinates(a, b)
    iou_record(core, out, "rect_64x65_sparse", a, b, T.cotangent(2, 64, 65, density=0.05))
    x, _ = T.clustered_pair(103, 41, 1)
    assert distinct_coordinates(x)
    iou_record(core, out, "self_41", x, None, T.cotangent(3, 41, 41))
    a, b = T.tie_boxes(104, 4)
    iou_record(core, out, "ties_20x20", a, b, T.cotangent(4, 20, 20))
    iou_record(core, out, "self_ties_20", a, None, T.cotangent(5, 20, 20))
    out["iou_cases"] = np.array(["rect_37x53", "rect_64x65_sparse", "self_41", "ties_20x20", "self_ties_20"])
    for tag in sorted(LAYER_CASES):
        layer_record(core, gn, out, tag, LAYER_CASES[tag], T)
    out["layer_cases"] = np.array(sorted(LAYER_CASES))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
