"""The heads assembly (groomed_nms_amd.heads, csrc/heads.hip) without a GPU: the C ABI and its argument checks, the wrapper's
ValueErrors, anchor_grid against the reference's tables, and a float64 NumPy restatement of the layout contract,
written from the contract and compared with every case of tests/golden/heads.npz -- what the reference's own RPN.forward and
torch.autograd.grad returned on the CPU (tests/golden/make_heads_golden.py).  test_heads_gpu.py reuses the restatement and `e_ref`.

e_ref: for the outputs that go through an exp (prob, the two sigmoid columns of bbox_3d, acceptance) and for the gradients that are
more than a copy (cls_map, axis, head, acceptance), the reference's float32 result differs from the float64 restatement by a handful
of roundings.  e_ref[name] is the largest such difference over all cases of the file; the HIP path is held to twice that."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = np.float64

# case -> (shape case whose maps and cotangents it uses, has the acceptance head, the cotangents it passes)
ALL_COT = ("cls", "prob", "bbox_2d", "bbox_3d", "acceptance")
CASES = {"s_1_1_1_1_2": ("s_1_1_1_1_2", True, ALL_COT), "s_2_3_5_7_4": ("s_2_3_5_7_4", True, ALL_COT),
         "s_2_36_2_9_4": ("s_2_36_2_9_4", True, ALL_COT), "s_1_2_3_130_3": ("s_1_2_3_130_3", True, ALL_COT),
         "no_acceptance": ("s_2_3_5_7_4", False, ALL_COT[:4]), "bbox_3d_only": ("s_2_3_5_7_4", True, ("bbox_3d",))}
MAP_NAMES = ("cls", "x", "y", "w", "h", "x3d", "y3d", "z3d", "w3d", "h3d", "l3d", "alpha", "axis", "head", "acceptance")
E_REF_NAMES = ("prob", "sigmoid_3d", "acceptance", "d_cls", "d_axis", "d_head", "d_acceptance")


@pytest.fixture(scope="module")
def gold():
    return Golden("heads.npz")


def case_maps(g, case):
    """the fifteen float32 maps of a case (the last one None without the acceptance head) and its C"""
    shape, has_acc, _ = CASES[case]
    maps = [g["%s/map_%s" % (shape, n)] for n in MAP_NAMES]
    if not has_acc:
        maps[-1] = None
    return maps, int(shape.split("_")[-1])


def case_cotangents(g, case):
    shape, _, which = CASES[case]
    return {n: (g["%s/g_%s" % (shape, n)] if n in which else None) for n in ALL_COT}


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement: the layout contract in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def np_sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def np_heads(maps, C):
    """maps: cls_map [B, C * A, H, W] (channel c * A + a), thirteen box maps [B, A, H, W], the acceptance map or None
    -> dict of float64 rows [B, R, .], R = A * H * W, row r = (a * H + h) * W + w"""
    B, _, H, W = maps[1].shape
    A = maps[1].shape[1]
    R = A * H * W
    logits = np.empty((B, R, C), F8)
    for c in range(C):
        logits[:, :, c] = maps[0].astype(F8).reshape(B, C * R)[:, c * R:(c + 1) * R]          # cls[b, r, c] = cls_map[b].flat[c R + r]
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    col = [m.astype(F8).reshape(B, R) for m in maps[1:14]]                                     # map_k[b].flat[r]
    out = dict(cls=logits, prob=e / e.sum(axis=2, keepdims=True), bbox_2d=np.stack(col[:4], axis=2),
               bbox_3d=np.stack(col[4:10] + [col[10], col[10], np_sigmoid(col[11]), np_sigmoid(col[12])], axis=2), acceptance=None)
    if maps[14] is not None:
        out["acceptance"] = np_sigmoid(maps[14].astype(F8).reshape(B, R, 1))
    return out


def np_heads_backward(fw, cot, maps, C):
    """fw: np_heads' result; cot: name -> cotangent rows or None (= zero) -> the fifteen maps' float64 gradients (None without the map)"""
    B, A, H, W = maps[1].shape
    R = A * H * W
    z = {n: (np.zeros(fw[n].shape) if cot.get(n) is None else cot[n].astype(F8)) for n in ALL_COT if fw[n] is not None}
    p = fw["prob"]
    d_rows = z["cls"] + p * (z["prob"] - (z["prob"] * p).sum(axis=2, keepdims=True))
    grads = [np.ascontiguousarray(d_rows.transpose(0, 2, 1)).reshape(B, C * A, H, W)]
    g2, g3 = z["bbox_2d"], z["bbox_3d"]
    s_axis, s_head = fw["bbox_3d"][:, :, 8], fw["bbox_3d"][:, :, 9]
    cols = [g2[:, :, k] for k in range(4)] + [g3[:, :, k] for k in range(6)]
    cols += [g3[:, :, 6] + g3[:, :, 7], g3[:, :, 8] * s_axis * (1 - s_axis), g3[:, :, 9] * s_head * (1 - s_head)]
    grads += [c.reshape(B, A, H, W) for c in cols]
    if fw["acceptance"] is None:
        grads.append(None)
    else:
        s = fw["acceptance"]
        grads.append((z["acceptance"] * s * (1 - s)).reshape(B, A, H, W))
    return grads


def reference_errors(g):
    """e_ref per name of E_REF_NAMES: max |the reference's float32 - the restatement| over every case of the file"""
    e = dict.fromkeys(E_REF_NAMES, 0.0)

    def up(name, ref, mine):
        e[name] = max(e[name], float(np.max(np.abs(ref.astype(F8) - mine))) if ref.size else 0.0)
    for case in CASES:
        maps, C = case_maps(g, case)
        fw = np_heads(maps, C)
        gr = np_heads_backward(fw, case_cotangents(g, case), maps, C)
        up("prob", g[case + "/prob"], fw["prob"])
        up("sigmoid_3d", g[case + "/bbox_3d"][:, :, 8:], fw["bbox_3d"][:, :, 8:])
        up("d_cls", g[case + "/d_cls"], gr[0])
        up("d_axis", g[case + "/d_axis"], gr[12])
        up("d_head", g[case + "/d_head"], gr[13])
        if maps[14] is not None:
            up("acceptance", g[case + "/acceptance"], fw["acceptance"])
            up("d_acceptance", g[case + "/d_acceptance"], gr[14])
    return e


# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_sources_and_reexport():
    import groomed_nms_amd
    from groomed_nms_amd import build, _lib, heads
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    for name in ("gnms_heads_assemble", "gnms_heads_assemble_backward"):
        assert "int %s(" % name in header and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "heads.hip" in build.SOURCES
    assert groomed_nms_amd.assemble_heads is heads.assemble_heads
    assert set(heads.__all__) >= {"assemble_heads", "anchor_grid", "Heads"}
    assert heads.Heads._fields == ("cls", "prob", "bbox_2d", "bbox_3d", "acceptance")
    assert lib.gnms_abi_version() == 1


def test_heads_py_stands_alone():
    text = open(os.path.join(ROOT, "groomed_nms_amd", "heads.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(tests|oracle|conftest)\b", text, flags=re.M)
    assert "tests/" not in text and "oracle" not in text


def test_library_argument_checks_without_gpu():
    from groomed_nms_amd import build, _lib
    build.build()
    lib = _lib.load()
    fake = 256 * 1024                             # never dereferenced: every check below returns before any HIP call
    maps = (ctypes.c_void_p * 15)(*[fake] * 15)
    strides = (ctypes.c_longlong * 15)(*[64] * 15)
    grads = (ctypes.c_void_p * 15)(*[fake] * 15)

    def fwd(**k):
        a = dict(maps=maps, strides=strides, B=1, A=2, H=3, W=4, C=4, cls=fake, prob=fake, b2=fake, b3=fake, acc=fake)
        a.update(k)
        return lib.gnms_heads_assemble(ctypes.addressof(a["maps"]) if a["maps"] is not None else None,
                                       ctypes.addressof(a["strides"]) if a["strides"] is not None else None, a["B"], a["A"], a["H"], a["W"],
                                       a["C"], a["cls"], a["prob"], a["b2"], a["b3"], a["acc"], None)

    def bwd(**k):
        a = dict(prob=fake, b3=fake, acc=fake, g_cls=fake, g_prob=fake, g_b2=fake, g_b3=fake, g_acc=fake, B=1, A=2, H=3, W=4, C=4, grads=grads)
        a.update(k)
        return lib.gnms_heads_assemble_backward(a["prob"], a["b3"], a["acc"], a["g_cls"], a["g_prob"], a["g_b2"], a["g_b3"], a["g_acc"], a["B"], a["A"],
                                                a["H"], a["W"], a["C"], ctypes.addressof(a["grads"]) if a["grads"] is not None else None, None)
    no_x = (ctypes.c_void_p * 15)(*([fake] + [None] + [fake] * 13))
    neg = (ctypes.c_longlong * 15)(*([64] * 3 + [-1] + [64] * 11))
    for bad in (dict(B=-1), dict(A=0), dict(H=0), dict(W=0), dict(A=-3), dict(maps=None), dict(strides=None), dict(maps=no_x), dict(strides=neg),
                dict(cls=None), dict(prob=None), dict(b2=None), dict(b3=None), dict(acc=None), dict(cls=fake + 4), dict(prob=fake + 8),
                dict(b2=fake + 4), dict(b3=fake + 8)):
        assert fwd(**bad) == -1 and lib.gnms_last_error(), bad
    assert fwd(B=0) == 0 and fwd(B=0, maps=None, cls=None) == 0
    for C in (1, 17, 0, -4):
        assert fwd(C=C) == -2 and b"2..16" in lib.gnms_last_error()
        assert bwd(C=C) == -2
    assert fwd(A=1 << 12, H=1 << 12, W=1 << 12) == -2                                       # R past 2^31
    for bad in (dict(B=-1), dict(A=0), dict(H=0), dict(W=0), dict(grads=None), dict(prob=None), dict(b3=None), dict(acc=None), dict(g_cls=fake + 4),
                dict(g_prob=fake + 8), dict(g_b2=fake + 4), dict(g_b3=fake + 8), dict(prob=fake + 4), dict(b3=fake + 4)):
        assert bwd(**bad) == -1 and lib.gnms_last_error(), bad
    assert bwd(B=0) == 0 and bwd(B=0, grads=None) == 0


def _maps(B=1, A=2, H=3, W=4, C=4, device="cpu"):
    return torch.zeros(B, C * A, H, W, device=device), [torch.zeros(B, A, H, W, device=device) for _ in range(13)], torch.zeros(B, A, H, W, device=device)


def test_wrapper_value_errors():
    from groomed_nms_amd import heads
    cls_map, box, acc = _maps()
    with pytest.raises(ValueError, match="GPU"):                                            # host tensors: no CPU fallback
        heads.assemble_heads(cls_map, box, acc)
    with pytest.raises(ValueError, match="GPU"):
        heads.assemble_heads(cls_map, box)
    for n in (12, 14, 0):
        with pytest.raises(ValueError, match="13"):
            heads.assemble_heads(cls_map, (box * 2)[:n], acc)
    for k in (0, 5, 12):                                                                    # shapes that disagree
        for shape in ((1, 2, 3, 5), (1, 3, 3, 4), (2, 2, 3, 4), (1, 2, 4, 4)):
            with pytest.raises(ValueError):
                heads.assemble_heads(cls_map, box[:k] + [torch.zeros(shape)] + box[k + 1:], acc)
    with pytest.raises(ValueError):
        heads.assemble_heads(cls_map, box, torch.zeros(1, 2, 3, 5))
    with pytest.raises(ValueError):
        heads.assemble_heads(torch.zeros(2, 8, 3, 4), box, acc)
    with pytest.raises(ValueError):
        heads.assemble_heads(torch.zeros(1, 8, 4, 3), box, acc)
    with pytest.raises(ValueError, match="multiple"):                                       # C * A not divisible by A
        heads.assemble_heads(torch.zeros(1, 7, 3, 4), box, acc)
    with pytest.raises(ValueError):
        heads.assemble_heads(torch.zeros(1, 8, 12), box, acc)
    with pytest.raises(ValueError):
        heads.assemble_heads(torch.zeros(1, 8, 3, 4, dtype=torch.int32), box, acc)
    with pytest.raises(ValueError):
        heads.assemble_heads(None, box, acc)


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_matches_reference(gold, case):
    maps, C = case_maps(gold, case)
    fw = np_heads(maps, C)
    assert np.array_equal(fw["cls"], gold[case + "/cls"].astype(F8))
    assert np.array_equal(fw["bbox_2d"], gold[case + "/bbox_2d"].astype(F8))
    assert np.array_equal(fw["bbox_3d"][:, :, :8], gold[case + "/bbox_3d"][:, :, :8].astype(F8))
    assert gold[case + "/bbox_3d"].shape[2] == 10 and gold[case + "/prob"].shape == fw["prob"].shape
    assert (fw["acceptance"] is None) == (not gold.has(case + "/acceptance"))
    np.testing.assert_allclose(gold[case + "/prob"], fw["prob"], rtol=0, atol=4e-7)
    np.testing.assert_allclose(gold[case + "/bbox_3d"][:, :, 8:], fw["bbox_3d"][:, :, 8:], rtol=0, atol=4e-7)
    cot = case_cotangents(gold, case)
    gr = np_heads_backward(fw, cot, maps, C)
    z3 = cot["bbox_3d"].astype(F8)
    for k, name in enumerate(MAP_NAMES):
        if gr[k] is None:
            assert name == "acceptance" and not gold.has(case + "/d_acceptance")
            continue
        ref = gold["%s/d_%s" % (case, name)]
        assert ref.shape == gr[k].shape and np.all(np.isfinite(ref))
        if name in ("cls", "axis", "head", "acceptance"):
            np.testing.assert_allclose(ref, gr[k], rtol=2e-6, atol=2e-6)
        elif name == "alpha":                                                              # one float32 addition
            want = (cot["bbox_3d"][:, :, 6] + cot["bbox_3d"][:, :, 7]).reshape(ref.shape)
            assert want.dtype == np.float32 and np.array_equal(ref, want)
        else:                                                                               # the cotangent column unchanged
            assert np.array_equal(ref.astype(F8), gr[k])
    assert z3.shape[2] == 10
    if case == "bbox_3d_only":
        assert not np.any(gold[case + "/d_cls"]) and not np.any(gr[0])


def test_goldens_cover_what_they_should(gold):
    shapes = {c: tuple(int(v) for v in c.split("_")[1:]) for c in CASES if c.startswith("s_")}
    assert set(shapes.values()) == {(1, 1, 1, 1, 2), (2, 3, 5, 7, 4), (2, 36, 2, 9, 4), (1, 2, 3, 130, 3)}
    for c, (B, A, H, W, C) in shapes.items():
        assert gold[c + "/map_cls"].shape == (B, C * A, H, W) and gold[c + "/map_head"].shape == (B, A, H, W)
    rows = gold["s_2_36_2_9_4/cls"].reshape(-1, 4)
    assert np.any(np.abs(rows) == 100) and np.any(np.all(rows == rows[:, :1], axis=1)), "no +-100 entries / no all-equal rows"
    assert np.any(np.abs(gold["s_1_2_3_130_3/cls"]) == 100)
    for case in CASES:
        for k in gold.keys:
            if k.startswith(case + "/"):
                assert np.all(np.isfinite(gold[k])), k
    e = reference_errors(gold)
    print("e_ref:", {k: "%.3g" % v for k, v in e.items()})
    assert all(v > 0 for v in e.values()), e
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "heads.npz")) < 1 << 20


@pytest.mark.parametrize("shape", [c for c in CASES if c.startswith("s_")])
def test_anchor_grid_matches_reference(gold, shape):
    from groomed_nms_amd import heads
    B, A, H, W, _ = (int(v) for v in shape.split("_")[1:])
    anchors, stride = gold[shape + "/anchors"], float(gold[shape + "/feat_stride"])
    got = heads.anchor_grid(anchors, (H, W), stride)
    for t, name in zip(got, ("rois", "rois_3d", "rois_2d_cen")):
        want = gold["%s/%s" % (shape, name)]
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want.shape
        assert t.numpy().tobytes() == want.tobytes(), name
    again = heads.anchor_grid(anchors.copy(), [H, W], stride)
    assert all(a is b for a, b in zip(got, again))                                          # cached per contents, not per object
    batched = heads.anchor_grid(anchors, (H, W), stride, batch=3)
    assert all(a is b for a, b in zip(batched, heads.anchor_grid(anchors, (H, W), stride, batch=3)))
    R = A * H * W
    for t, base in zip(batched, got):
        assert t.shape[0] == 3 and t.is_contiguous() and t.stride(0) == R * t.stride(1) and all(torch.equal(t[b], base) for b in range(3))
    other = heads.anchor_grid(anchors + 1.0, (H, W), stride)
    assert other[0] is not got[0] and not torch.equal(other[0], got[0])
    assert heads.anchor_grid(anchors, (H, W), stride + 1)[0] is not got[0]
    with pytest.raises(ValueError):
        heads.anchor_grid(anchors[:, :3], (H, W), stride)


def test_anchor_grid_cache_is_bounded():
    """feature sizes that vary (inference on images of many sizes) do not pile up tables: the least recently used set goes"""
    from groomed_nms_amd import heads
    anchors = np.array([[-8.0, -8.0, 8.0, 8.0, 1.0], [-4.0, -12.0, 4.0, 12.0, 2.0]])
    first = heads.anchor_grid(anchors, (1, 1), 16.0)
    for w in range(2, heads.GRID_CACHE_ENTRIES + 2):
        heads.anchor_grid(anchors, (1, w), 16.0)
        assert len(heads._GRIDS) <= heads.GRID_CACHE_ENTRIES
    again = heads.anchor_grid(anchors, (1, 1), 16.0)
    assert again[0] is not first[0] and all(torch.equal(a, b) for a, b in zip(first, again))
    assert heads.anchor_grid(anchors, (1, 1), 16.0)[0] is again[0]
