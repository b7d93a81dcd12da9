"""The heads assembly on the GPU (groomed_nms_amd.heads, csrc/heads.hip) against tests/golden/heads.npz and the float64 restatement of
test_heads_host.py: the pure-layout outputs and gradients bit for bit, the ones behind an exp within 2 x e_ref of the restatement --
e_ref being the reference's own float32 distance from the same restatement over the whole file, and 2 because both are a handful of
roundings in a different order and neither is the correct one.  Every comparison prints its ratio error / e_ref before it asserts."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import Golden
from test_heads_host import ALL_COT, CASES, MAP_NAMES, case_cotangents, case_maps, np_heads, np_heads_backward, reference_errors

pytestmark = pytest.mark.gpu
F8 = np.float64


@pytest.fixture(scope="module")
def gold():
    return Golden("heads.npz")


@pytest.fixture(scope="module")
def e_ref(gold):
    return reference_errors(gold)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _leaves(maps, dev):
    return [torch.from_numpy(m.copy()).to(dev).requires_grad_(True) if m is not None else None for m in maps]


def _run(maps, cot, dev, leaves=None):
    """assemble_heads and its gradients for the cotangents `cot` (name -> array or None) -> (Heads of arrays, list of 15 gradient arrays)"""
    from groomed_nms_amd import heads
    leaves = _leaves(maps, dev) if leaves is None else leaves
    out = heads.assemble_heads(leaves[0], leaves[1:14], leaves[14])
    names = [n for n in ALL_COT if cot.get(n) is not None]
    used = [t for t in leaves if t is not None]
    grads = torch.autograd.grad([getattr(out, n) for n in names], used, [torch.from_numpy(cot[n]).to(dev) for n in names], allow_unused=True)
    torch.cuda.synchronize()
    grads = [g.cpu().numpy() if g is not None else None for g in grads] + [None] * (15 - len(used))
    return heads.Heads(*[t.detach().cpu().numpy() if t is not None else None for t in out]), grads


def _ratio(what, got, want64, e):
    err = float(np.max(np.abs(got.astype(F8) - want64)))
    print("%s: max error %.3g, e_ref %.3g, ratio %.3f" % (what, err, e, err / e))
    return err


@pytest.mark.parametrize("case", list(CASES))
def test_golden_case(gold, e_ref, dev, case):
    maps, C = case_maps(gold, case)
    cot = case_cotangents(gold, case)
    out, grads = _run(maps, cot, dev)
    fw = np_heads(maps, C)
    gr = np_heads_backward(fw, cot, maps, C)
    for t in out:
        assert t is None or (t.dtype == np.float32 and np.all(np.isfinite(t)))
    assert out.cls.tobytes() == gold[case + "/cls"].tobytes()
    assert out.bbox_2d.tobytes() == gold[case + "/bbox_2d"].tobytes()
    assert out.bbox_3d.shape == gold[case + "/bbox_3d"].shape
    assert np.ascontiguousarray(out.bbox_3d[:, :, :8]).tobytes() == np.ascontiguousarray(gold[case + "/bbox_3d"][:, :, :8]).tobytes()
    errs = [(_ratio(case + " prob", out.prob, fw["prob"], e_ref["prob"]), e_ref["prob"]),
            (_ratio(case + " bbox_3d[8:]", out.bbox_3d[:, :, 8:], fw["bbox_3d"][:, :, 8:], e_ref["sigmoid_3d"]), e_ref["sigmoid_3d"])]
    if maps[14] is None:
        assert out.acceptance is None and grads[14] is None
    else:
        assert out.acceptance.shape == gold[case + "/acceptance"].shape
        errs.append((_ratio(case + " acceptance", out.acceptance, fw["acceptance"], e_ref["acceptance"]), e_ref["acceptance"]))
    g3 = cot["bbox_3d"]
    for k, name in enumerate(MAP_NAMES):
        if gr[k] is None:
            continue
        assert grads[k] is not None and grads[k].dtype == np.float32 and grads[k].shape == gr[k].shape and np.all(np.isfinite(grads[k])), name
        if name in ("cls", "axis", "head", "acceptance"):
            errs.append((_ratio("%s d_%s" % (case, name), grads[k], gr[k], e_ref["d_" + name]), e_ref["d_" + name]))
        elif name == "alpha":
            assert grads[k].tobytes() == (g3[:, :, 6] + g3[:, :, 7]).astype(np.float32).tobytes()
        else:
            assert grads[k].tobytes() == gr[k].astype(np.float32).tobytes(), name            # the cotangent column, or zeros
    for err, e in errs:
        assert err <= 2 * e
    if case == "bbox_3d_only":
        assert not np.any(grads[0]) and not np.any(grads[1]) and not np.any(grads[14])


def test_channel_slices_of_a_stacked_tensor(gold, dev):
    """maps that are channel slices of one stacked [B, (C + 14) A + pad, H, W] tensor: batch stride != A H W, nothing copied"""
    case = "s_2_36_2_9_4"
    maps, C = case_maps(gold, case)
    cot = case_cotangents(gold, case)
    want, want_grads = _run(maps, cot, dev)
    pad = np.zeros_like(maps[1][:, :5])
    stacked = torch.from_numpy(np.concatenate([pad] + maps + [pad], axis=1)).to(dev)
    leaves, at = [], 5
    for m in maps:                  # each slice a leaf of its own: autograd's sum into one stacked gradient would turn -0.0 into +0.0
        leaves.append(stacked[:, at:at + m.shape[1]].requires_grad_(True))
        at += m.shape[1]
    assert all(t.stride(0) == stacked.stride(0) != t.shape[1] * t.shape[2] * t.shape[3] and not t.is_contiguous() for t in leaves)
    assert all(t.data_ptr() != leaves[0].data_ptr() and t.untyped_storage().data_ptr() == stacked.untyped_storage().data_ptr() for t in leaves[1:])
    got, got_grads = _run(maps, cot, dev, leaves)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and all(a.tobytes() == b.tobytes() for a, b in zip(got_grads, want_grads))
    # the same through one stacked leaf: autograd adds the slices' gradients into one tensor
    stacked.requires_grad_(True)
    views, at = [], 5
    for m in maps:
        views.append(stacked[:, at:at + m.shape[1]])
        at += m.shape[1]
    from groomed_nms_amd import heads
    out = heads.assemble_heads(views[0], views[1:14], views[14])
    g, = torch.autograd.grad(list(out), [stacked], [torch.from_numpy(cot[n]).to(dev) for n in ALL_COT])
    g = g.cpu().numpy()
    assert not np.any(g[:, :5]) and not np.any(g[:, at:])
    assert np.array_equal(g[:, 5:at], np.concatenate(want_grads, axis=1))
    # a map that is not block-contiguous (channels last) is copied; same bits
    leaves = _leaves(maps, dev)
    leaves[0] = leaves[0].detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    leaves[7] = leaves[7].detach().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    got, got_grads = _run(maps, cot, dev, leaves)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and all(a.tobytes() == b.tobytes() for a, b in zip(got_grads, want_grads))


def test_two_runs_are_bit_identical_and_other_dtypes(gold, dev):
    case = "s_1_2_3_130_3"
    maps, C = case_maps(gold, case)
    cot = case_cotangents(gold, case)
    a, ga = _run(maps, cot, dev)
    b, gb = _run(maps, cot, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and all(x.tobytes() == y.tobytes() for x, y in zip(ga, gb))
    # float64 maps (the golden's values are exact in it): converted on input, the gradient comes back in the map's dtype
    leaves = [t.detach().double().requires_grad_(True) for t in _leaves(maps, dev)]
    from groomed_nms_amd import heads
    out = heads.assemble_heads(leaves[0], leaves[1:14], leaves[14])
    assert all(t.dtype == torch.float32 for t in out)
    grads = torch.autograd.grad(list(out), leaves, [torch.from_numpy(cot[n]).to(dev) for n in ALL_COT])
    assert all(g.dtype == torch.float64 for g in grads)
    assert all(x.tobytes() == y.detach().cpu().numpy().tobytes() for x, y in zip(a, out))
    assert all(x.tobytes() == y.float().cpu().numpy().tobytes() for x, y in zip(ga, grads))


_ROW_STORES_CASES = ("s_2_36_2_9_4", "s_1_2_3_130_3")

_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, "tests")
import test_heads_gpu as T
gold, dev = T.Golden("heads.npz"), torch.device("cuda", torch.cuda.current_device())
res = {}
for case in T._ROW_STORES_CASES:
    out, _ = T._run(T.case_maps(gold, case)[0], T.case_cotangents(gold, case), dev)
    res.update({"%s/%s" % (case, n): v for n, v in out._asdict().items()})
np.savez(sys.argv[1], **res)
"""


def test_row_stores_switch_writes_the_same_bits(gold, dev):
    """GNMS_HEADS_ROW_STORES=1 (developer A/B switch, read once, hence one fresh child process): per-lane row stores instead of the LDS
    tile copy write the same bits"""
    assert os.environ.get("GNMS_HEADS_ROW_STORES", "0") != "1", "the suite tests the default stores"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rows.npz")
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, path], cwd=root, env=dict(os.environ, GNMS_HEADS_ROW_STORES="1"),
                           capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(path) as z:
            rows = {k: z[k] for k in z.files}
    for case in _ROW_STORES_CASES:
        out, _ = _run(case_maps(gold, case)[0], case_cotangents(gold, case), dev)
        for n, v in out._asdict().items():
            assert rows["%s/%s" % (case, n)].tobytes() == v.tobytes(), (case, n)


def test_no_grad_saves_nothing_and_bbox_2d_may_be_scaled_in_place(gold, dev):
    from groomed_nms_amd import heads
    maps, C = case_maps(gold, "s_2_3_5_7_4")
    leaves = _leaves(maps, dev)
    with torch.no_grad():
        out = heads.assemble_heads(leaves[0], leaves[1:14], leaves[14])
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    out = heads.assemble_heads(leaves[0], leaves[1:14], leaves[14])
    plain = out.bbox_2d.detach().clone()
    out.bbox_2d[:, :, 0] *= 2.0                                      # what rpn_util.py:902-912 does to the returned tensor
    out.cls.mul_(1.0)
    (out.bbox_2d.sum() + out.prob.sum() + out.bbox_3d.sum() + out.acceptance.sum() + out.cls.sum()).backward()
    assert torch.equal(out.bbox_2d[:, :, 1:].detach(), plain[:, :, 1:]) and torch.equal(leaves[1].grad, torch.full_like(leaves[1], 2.0))
    assert torch.equal(leaves[2].grad, torch.ones_like(leaves[2])) and torch.equal(leaves[11].grad, torch.full_like(leaves[11], 2.0))
    out = heads.assemble_heads(leaves[0], leaves[1:14], leaves[14])
    out.bbox_3d.mul_(2.0)                                             # a saved output: autograd's version check refuses the backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.bbox_3d.sum().backward()


def test_graph_capture_replays_with_new_contents(gold, dev):
    from groomed_nms_amd import heads
    case = "s_2_36_2_9_4"
    maps, C = case_maps(gold, case)
    cot = case_cotangents(gold, case)
    rng = np.random.default_rng(5)
    other = [rng.normal(0, 1.5, m.shape).astype(np.float32) for m in maps]
    eager = [_run(m, cot, dev) for m in (maps, other)]
    static = _leaves(maps, dev)
    gs = [torch.from_numpy(cot[n]).to(dev) for n in ALL_COT]

    def step():
        out = heads.assemble_heads(static[0], static[1:14], static[14])
        return list(out) + list(torch.autograd.grad(list(out), static, gs))
    step()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = step()
    torch.cuda.synchronize()
    for contents, (want, want_grads) in ((other, eager[1]), (maps, eager[0])):
        with torch.no_grad():
            for t, m in zip(static, contents):
                t.copy_(torch.from_numpy(m))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().cpu().numpy() for t in outs]
        for i, (a, b) in enumerate(zip(got, list(want) + want_grads)):
            assert a.tobytes() == b.tobytes(), "output %d" % i


def test_too_many_classes_is_unsupported(dev):
    from groomed_nms_amd import heads
    from groomed_nms_amd._lib import GnmsError
    z = lambda ch: torch.zeros(1, ch, 2, 3, device=dev)              # noqa: E731
    with pytest.raises(GnmsError, match=r"\(-2\)"):
        heads.assemble_heads(z(17 * 2), [z(2) for _ in range(13)], z(2))
    with pytest.raises(GnmsError, match=r"\(-2\)"):
        heads.assemble_heads(z(2), [z(2) for _ in range(13)])         # C = 1
    out = heads.assemble_heads(z(16 * 2), [z(2) for _ in range(13)])
    assert out.prob.shape == (1, 12, 16) and out.acceptance is None and torch.all(out.prob == 1.0 / 16)


def test_anchor_grid_on_the_device(gold, dev):
    from groomed_nms_amd import heads
    shape = "s_2_36_2_9_4"
    anchors, stride = gold[shape + "/anchors"], float(gold[shape + "/feat_stride"])
    R = 36 * 2 * 9
    tables = heads.anchor_grid(anchors, (2, 9), stride, batch=2, device=dev)
    assert all(a is b for a, b in zip(tables, heads.anchor_grid(anchors, (2, 9), stride, batch=2, device=dev)))
    for t, name, cols in zip(tables, ("rois", "rois_3d", "rois_2d_cen"), (5, 11, 2)):
        assert t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == (2, R, cols)
        assert t.stride(2) == 1 and t.stride(1) >= cols and t.stride(0) == R * t.stride(1)          # regression._rows reads it where it lies
        want = gold["%s/%s" % (shape, name)]
        assert all(t[b].cpu().numpy().tobytes() == want.tobytes() for b in range(2))
    from groomed_nms_amd.regression import _rows
    for t, cols in zip(tables, (4, 11, 2)):
        assert _rows(t, dev, 2, R, cols, "table")[0].data_ptr() == t.data_ptr()
