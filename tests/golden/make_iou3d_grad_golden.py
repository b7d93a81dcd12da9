"""Generate tests/golden/iou3d_grad.npz by IMPORTING the reference's lib/math_3d.py, lib/core.py and lib/groomed_nms.py and letting torch
autograd differentiate them in float32 on the CPU.  Runs only where the reference checkout is (the first argument, read-only); it
writes data only.

  overlap/<tag>/{a, b, cotangent, method, ext_a, ext_b, grad_a, grad_b}
        f(iou3d_approximate(get_corners_of_cuboid(a), get_corners_of_cuboid(b), "combinations", ...)).backward(cotangent) w.r.t. the
        seven parameters; method 0 normal, 1 generalized, 2 0.5 (1 + generalized) (lib/loss/rpn_3d.py:781); rectangular 37 x 53 in all
        three methods, 64 x 65 under a 5 %-dense cotangent, self 41 (b absent: the same corners on both sides).  ext_*: the extents
        (x0, x1, y0, y1, z0, z1) of the reference's own float32 corners -- what its float32 arithmetic saw.
  layer/<tag>/{seed, params, scores, weights, ext, params_grad, kw/...}
        differentiable_nms(scores, 0.5 (1 + generalized overlap of params with itself), **kw)[2] with params.requires_grad, N = 60,
        loss = sum(weights * prob): default, group cap 5, unmasked groups, ungrouped, sigmoidal pruning

The inputs come from the builders of tests/test_iou3d_grad_host.py (seeded NumPy, synthetic.boxes_3d), so the file regenerates bit for
bit.  Conditions on the reference, asserted here: every |sin ry| and |cos ry| is at least 1e-3 (no corner ties); no two boxes share an
extent edge; every box is sane by record_bad_flag's definition (extents in (1e-4, 1e5), coordinates below 1e5); no overlap within 8 eps
of nms_threshold; no rescored probability within 8 eps of the valid-box threshold or of a clamp bound (exact 0 and 1 apart).

usage: python tests/golden/make_iou3d_grad_golden.py REFERENCE_CHECKOUT"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_iou_grad_golden as M2                                     # noqa: E402  (the reference loader and its stubs)

OUT = os.path.join(HERE, "iou3d_grad.npz")
EPS = M2.EPS
N_LAYER = 60
LAYER_CASES = M2.LAYER_CASES
DEFAULTS = M2.DEFAULTS


def conditions(tag, *param_sets, exts):
    p = np.concatenate(param_sets, 0).astype(np.float64)
    assert (np.abs(np.sin(p[:, 6])) >= 1e-3).all() and (np.abs(np.cos(p[:, 6])) >= 1e-3).all(), "%s: a corner tie" % tag
    e = np.concatenate(exts, 0)
    for ax in (0, 1, 2):
        v = np.concatenate([e[:, 2 * ax], e[:, 2 * ax + 1]])
        assert len(np.unique(v)) == len(v), "%s: two boxes share an extent edge" % tag
        ln = e[:, 2 * ax + 1] - e[:, 2 * ax]
        assert ((ln > 1e-4) & (ln < 1e5)).all(), "%s: a box is not sane" % tag
    assert (np.abs(e) < 1e5).all(), "%s: a box is not sane" % tag


def overlap_of(math_3d, core, ta, tb, method):
    """the reference's functions on parameter tensors [n, 7]; returns (overlap, float32 extents of a, of b)"""
    from test_iou3d_grad_host import extents_of_corners
    ca = math_3d.get_corners_of_cuboid(*ta.unbind(1))
    cb = ca if tb is None else math_3d.get_corners_of_cuboid(*tb.unbind(1))
    ea, eb = extents_of_corners(ca.detach().numpy()), extents_of_corners(cb.detach().numpy())
    # (iou3d_approximate overwrites the y row of the corners it is given, lib/core.py:379: it gets its own copies)
    q = core.iou3d_approximate(ca.clone(), cb.clone(), mode="combinations", method="normal" if method == 0 else "generalized")[1]
    return (q if method < 2 else 0.5 * (1.0 + q)), ea, eb


def overlap_record(math_3d, core, out, tag, a, b, g, method):
    ta = torch.tensor(a, requires_grad=True)
    tb = None if b is None else torch.tensor(b, requires_grad=True)
    q, ea, eb = overlap_of(math_3d, core, ta, tb, method)
    conditions(tag, *([a] if b is None else [a, b]), exts=[ea] if b is None else [ea, eb])
    q.backward(torch.tensor(g))
    assert bool(torch.isfinite(ta.grad).all()) and bool(ta.grad.any()), tag
    out["overlap/%s/a" % tag] = a
    out["overlap/%s/ext_a" % tag] = ea.astype(np.float32)
    out["overlap/%s/cotangent" % tag] = g
    out["overlap/%s/method" % tag] = np.array(method)
    out["overlap/%s/grad_a" % tag] = ta.grad.numpy().copy()
    if b is not None:
        out["overlap/%s/b" % tag] = b
        out["overlap/%s/ext_b" % tag] = eb.astype(np.float32)
        out["overlap/%s/grad_b" % tag] = tb.grad.numpy().copy()


def layer_record(math_3d, core, gn, out, tag, kw):
    """the first seed of the case's own sequence whose inputs meet the conditions (deterministic: the same seed every run)"""
    for attempt in range(32):
        try:
            return layer_record_at(math_3d, core, gn, out, tag, kw, 16000 + 100 * sorted(LAYER_CASES).index(tag) + attempt)
        except AssertionError as e:
            print("layer/%s: seed +%d rejected (%s)" % (tag, attempt, e))
    raise AssertionError("%s: no seed meets the conditions" % tag)


def layer_record_at(math_3d, core, gn, out, tag, kw, seed):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    params = synthetic.boxes_3d(rng, N_LAYER, clustered=True, per=10)
    scores = synthetic.tie_free_scores(rng, N_LAYER)
    weights = rng.uniform(-1, 2, size=N_LAYER).astype(np.float32)
    k = dict(DEFAULTS)
    k.update(kw)
    tp = torch.tensor(params, requires_grad=True)
    m, ext, _ = overlap_of(math_3d, core, tp, None, 2)
    conditions(tag, params, exts=[ext])
    assert float((m.detach() - k["nms_threshold"]).abs().min()) > 8 * EPS, "%s: an overlap sits within 8 eps of nms_threshold" % tag
    probe = gn.differentiable_nms(torch.tensor(scores), m.detach(), **dict(k, valid_box_prob_threshold=0.0))[2].numpy()
    inside = probe[(probe != 0.0) & (probe != 1.0)]
    for bound in (0.0, 1.0, k["valid_box_prob_threshold"]):
        assert not len(inside) or float(np.abs(inside - bound).min()) > 8 * EPS, "%s: a rescored probability sits within 8 eps of %g" % (tag, bound)
    prob = gn.differentiable_nms(torch.tensor(scores), m, **k)[2]
    (prob * torch.tensor(weights)).sum().backward()
    assert tp.grad is not None and bool(torch.isfinite(tp.grad).all()) and bool(tp.grad.any()), tag
    out["layer/%s/seed" % tag] = np.array(seed)
    out["layer/%s/params" % tag] = params
    out["layer/%s/scores" % tag] = scores
    out["layer/%s/weights" % tag] = weights
    out["layer/%s/ext" % tag] = ext.astype(np.float32)
    out["layer/%s/params_grad" % tag] = tp.grad.numpy().copy()
    for key, v in kw.items():
        out["layer/%s/kw/%s" % (tag, key)] = np.array(v)


def main():
    M2.REF = sys.argv[1] if len(sys.argv) > 1 else None
    assert M2.REF and os.path.isdir(M2.REF), __doc__
    torch.manual_seed(0)
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.dirname(HERE))                          # tests/: the case builders
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))         # the repository: groomed_nms_amd.synthetic
    import test_iou3d_grad_host as T
    core, gn = M2.load_reference()
    import lib.math_3d as math_3d
    out, tags = {}, []
    a, b = T.clustered_pair3d(1101, 37, 53)
    for method in (2, 0, 1):
        tags.append("rect_37x53" if method == 2 else "rect_37x53_method%d" % method)
        overlap_record(math_3d, core, out, tags[-1], a, b, T.cotangent3d(1, 37, 53), method)
    a, b = T.clustered_pair3d(1102, 64, 65)
    overlap_record(math_3d, core, out, "rect_64x65_sparse", a, b, T.cotangent3d(2, 64, 65, density=0.05), 2)
    x, _ = T.clustered_pair3d(1103, 41, 1)
    overlap_record(math_3d, core, out, "self_41", x, None, T.cotangent3d(3, 41, 41), 2)
    out["overlap_cases"] = np.array(tags + ["rect_64x65_sparse", "self_41"])
    for tag in sorted(LAYER_CASES):
        layer_record(math_3d, core, gn, out, tag, LAYER_CASES[tag])
    out["layer_cases"] = np.array(sorted(LAYER_CASES))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
