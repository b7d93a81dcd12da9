"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the golden vectors
captured from the reference.  Run on the MI355X box with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from conftest import MODES, TOL, check_index_lists  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import groomed_nms_amd as g
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return g


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _run_gpu(G, s, m, w, want_gi, **kw):
    st = torch.from_numpy(s).cuda().requires_grad_(True)
    mt = torch.from_numpy(m).cuda().requires_grad_(bool(want_gi))
    valid, invalid, prob = G.differentiable_nms(st, mt, **kw)
    out = dict(valid=valid.cpu().numpy(), invalid=invalid.cpu().numpy(), prob=prob.detach().cpu().numpy())
    if len(s) and prob.requires_grad:
        (prob * torch.from_numpy(w).cuda()).sum().backward()
        out["grad_scores"] = st.grad.cpu().numpy()
        if want_gi:
            out["grad_iou"] = mt.grad.cpu().numpy()
    return out


def _golden_cases(g):
    out = []
    for case in g.cases():
        if not g.has(f"{case}/scores"):
            continue
        for mode in g.modes(case):
            if mode in MODES:
                out.append((case, mode))
    return out


def _check_case(G, O, g, case, mode):
    s, m, w = g[f"{case}/scores"], g[f"{case}/iou"], g[f"{case}/w"]
    want_gi = g.has(f"{case}/{mode}/grad_iou")
    res = _run_gpu(G, s, m, w, want_gi, **MODES[mode])
    # (1) against the reference's own outputs
    np.testing.assert_allclose(res["prob"], g[f"{case}/{mode}/prob"], atol=TOL, rtol=0, equal_nan=True)
    check_index_lists(res["valid"], res["invalid"], g[f"{case}/{mode}/valid"], g[f"{case}/{mode}/invalid"])
    if g.has(f"{case}/{mode}/grad_scores"):
        np.testing.assert_allclose(res["grad_scores"], g[f"{case}/{mode}/grad_scores"], atol=2e-4, rtol=1e-4)
    if want_gi:
        np.testing.assert_allclose(res["grad_iou"], g[f"{case}/{mode}/grad_iou"], atol=2e-4, rtol=1e-4)
    # (2) against the oracle: default (masked) mode is bit-exact
    ref = O.differentiable_nms(s, m, grad_prob=w if len(s) else None, want_grad_iou=want_gi, **MODES[mode])
    if mode.startswith("gm_lin"):     # linear pruning has no transcendental: bit-exact; expf differs by an ulp device vs libm
        assert np.array_equal(res["prob"], ref["prob"], equal_nan=True), f"{case}/{mode} prob not bit-exact"
        assert list(res["valid"]) == list(ref["valid"]) and list(res["invalid"]) == list(ref["invalid"])
        if len(s):
            assert np.array_equal(res["grad_scores"], ref["grad_scores"]), f"{case}/{mode} grad not bit-exact"
    else:
        np.testing.assert_allclose(res["prob"], ref["prob"], atol=TOL, rtol=0, equal_nan=True)


def test_nms_golden_small(G, O, golden_nms):
    cases = _golden_cases(golden_nms)
    assert len(cases) > 100
    for case, mode in cases:
        try:
            _check_case(G, O, golden_nms, case, mode)
        except AssertionError as e:
            raise AssertionError(f"{case}/{mode}: {e}") from e


def test_nms_golden_box_derived(G, O, golden_box2d, golden_box3d):
    for g in (golden_box2d, golden_box3d):
        for case, mode in _golden_cases(g):
            try:
                _check_case(G, O, g, case, mode)
            except AssertionError as e:
                raise AssertionError(f"{case}/{mode}: {e}") from e


def test_known_answer_vectors(G, golden_nms):
    """test/test_differentiable_nms_forward.py:127-140."""
    for case, v, iv in (("kat1", [0, 1, 3], [2]), ("kat2", [0, 1, 4], [2, 3])):
        valid, invalid, prob = G.differentiable_nms(torch.from_numpy(golden_nms[f"{case}/scores"]).cuda(),
                                                    torch.from_numpy(golden_nms[f"{case}/iou"]).cuda(), temperature=0.1)
        np.testing.assert_allclose(prob.cpu().numpy(), golden_nms[f"{case}/expected_prob"], atol=5e-4)
        assert valid.tolist() == v and sorted(invalid.tolist()) == iv


def test_numpy_in_cpu_out(G, golden_nms):
    """lib/rpn_util.py:1319-1320: NumPy float64 in, `.numpy()` on the index result."""
    s = golden_nms["kat2/scores"].astype(np.float64)
    m = golden_nms["kat2/iou"].astype(np.float64)
    valid, invalid, prob = G.differentiable_nms(s, m)
    assert valid.device.type == "cpu" and prob.device.type == "cpu"
    assert valid.numpy().tolist() == [0, 1, 4]


def test_iou2d_bit_exact(G, O, golden_box2d):
    from groomed_nms_amd import overlaps
    for case in ("uni64", "clu64", "uni256", "clu256", "clu250"):
        b = torch.from_numpy(golden_box2d[f"{case}/boxes"]).cuda()
        got = overlaps.iou(b, b).cpu().numpy()
        assert np.array_equal(got, golden_box2d[f"{case}/iou"], equal_nan=True), case
    got = overlaps.iou(golden_box2d["rect/a"], golden_box2d["rect/b"])          # ndarray in -> ndarray out
    assert isinstance(got, np.ndarray) and np.array_equal(got, golden_box2d["rect/iou"])
    z = overlaps.iou(torch.from_numpy(golden_box2d["zero_area/boxes"]).cuda(), torch.from_numpy(golden_box2d["zero_area/boxes"]).cuda())
    assert np.array_equal(z.cpu().numpy(), golden_box2d["zero_area/iou"], equal_nan=True)
    # odd sizes / unaligned leading dimension against the oracle
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(5)
    for M, N in ((1, 1), (3, 7), (65, 129), (257, 1023), (1000, 1001)):
        a, b = synthetic.uniform_boxes_2d(rng, M), synthetic.clustered_boxes_2d(rng, N, 8)
        got = overlaps.iou(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        assert np.array_equal(got, O.iou2d(a, b), equal_nan=True), (M, N)


def test_iou3d(G, O, golden_box3d):
    from groomed_nms_amd import overlaps
    g = golden_box3d
    for case in ("m5", "uni64", "clu64", "clu200"):
        p = g[f"{case}/params"]
        c = overlaps.get_corners_of_cuboid(*[torch.from_numpy(np.ascontiguousarray(p[:, i])).cuda() for i in range(7)])
        np.testing.assert_allclose(c.cpu().numpy(), g[f"{case}/corners"], atol=2e-5, rtol=1e-6)
        ref_c = torch.from_numpy(g[f"{case}/corners"]).cuda()
        keep = ref_c.clone()
        for method in ("normal", "generalized"):
            bev, i3 = overlaps.iou3d_approximate(ref_c, ref_c, mode="combinations", method=method)
            np.testing.assert_allclose(bev.cpu().numpy(), g[f"{case}/{method}/iou_bev"], atol=1e-6, rtol=1e-6)
            np.testing.assert_allclose(i3.cpu().numpy(), g[f"{case}/{method}/iou_3d"], atol=1e-6, rtol=1e-6)
            ob, o3 = O.iou3d_approximate(g[f"{case}/corners"], g[f"{case}/corners"], generalized=(method == "generalized"))
            assert np.array_equal(i3.cpu().numpy(), o3, equal_nan=True) and np.array_equal(bev.cpu().numpy(), ob, equal_nan=True)
        assert torch.equal(ref_c, keep)                                          # inputs are const (unlike lib/core.py:379-380)
        pt = torch.from_numpy(p).cuda().unsqueeze(0)
        exact = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True)[0]             # no threshold given: the exact operation order
        np.testing.assert_allclose(exact.cpu().numpy(), g[f"{case}/nms_overlap"], atol=TOL)
        assert torch.equal(exact, 0.5 * (1.0 + overlaps.iou3d_batched(pt, from_params=True, method="generalized")[0]))
        # the HBM-bound NMS-overlap kernel re-associates 0.5*(1+giou) (one reciprocal instead of two divisions): within a few ulp of
        # the exact-order kernel on the same records everywhere, and EQUAL to it inside the guard band around the threshold, so that
        # `> thr` takes the same decision for every pair
        for thr in (0.4, 0.25, 0.6):
            ov = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True, nms_threshold=thr)[0]
            np.testing.assert_allclose(ov.cpu().numpy(), exact.cpu().numpy(), atol=2e-6, rtol=0)
            assert torch.equal(ov > thr, exact > thr) and torch.equal(ov <= thr, exact <= thr), (case, thr)
            band = (exact - thr).abs() <= 4e-6
            assert torch.equal(ov[band], exact[band])
    bev, i3 = overlaps.iou3d_approximate(torch.from_numpy(g["rect/corners_a"]).cuda(), torch.from_numpy(g["rect/corners_b"]).cuda(),
                                         mode="combinations", method="generalized")
    np.testing.assert_allclose(i3.cpu().numpy(), g["rect/iou_3d"], atol=1e-6)
    np.testing.assert_allclose(bev.cpu().numpy(), g["rect/iou_bev"], atol=1e-6)


def test_get_groups(G, golden_nms, golden_box2d):
    for g in (golden_nms, golden_box2d):
        for case in g.cases():
            for gs in (100, 2):
                if not g.has(f"{case}/groups_gs{gs}/lens"):
                    continue
                s, m = g[f"{case}/scores"], g[f"{case}/iou"]
                order = np.argsort(-s, kind="stable")
                # the goldens were taken on the score-sorted problem, as differentiable_nms calls get_groups (:85)
                groups = G.get_groups(torch.from_numpy(m[order][:, order]).cuda(), 0.4, torch.from_numpy(s[order]).cuda(), group_size=gs)
                assert [len(x) for x in groups] == list(g[f"{case}/groups_gs{gs}/lens"]), (case, gs)
                flat = [int(v) for x in groups for v in x.tolist()]
                assert flat == list(g[f"{case}/groups_gs{gs}/flat"]), (case, gs)
                # unsorted input: same groups in original indices / in rank positions
                g2 = G.get_groups(torch.from_numpy(m).cuda(), 0.4, torch.from_numpy(s).cuda(), group_size=gs)
                assert [int(v) for x in g2 for v in x.tolist()] == [int(order[i]) for i in flat], (case, gs)
                g3 = G.get_groups(torch.from_numpy(m).cuda(), 0.4, torch.from_numpy(s).cuda(), group_size=gs, return_original_indices=False)
                assert [int(v) for x in g3 for v in x.tolist()] == flat, (case, gs)


def test_pruning_function(G, golden_misc):
    g = golden_misc
    x = torch.from_numpy(g["prune/x"]).cuda()
    for method, temp in (("linear", 0.01), ("sigmoidal", 0.1), ("sigmoidal", 0.01), ("soft_nms", 0.5), ("soft_nms", 0.1)):
        got = G.pruning_function(x, 0.4, temp, method).cpu().numpy()
        np.testing.assert_allclose(got, g[f"prune/{method}_{temp}/torch"], atol=1e-6)
        np.testing.assert_allclose(G.pruning_function(g["prune/x"][0].astype(np.float64), 0.4, temp, method),
                                   g[f"prune/{method}_{temp}/numpy_row0"], atol=1e-12)
    with pytest.raises(NotImplementedError):
        G.pruning_function(x, 0.4, 0.1, "bogus")
    with pytest.raises(NotImplementedError):
        G.differentiable_nms(torch.rand(4).cuda(), torch.eye(4).cuda(), pruning_method="bogus")


def _record(name, obj):
    """append one JSON line to gpurun_out/<name> (figures the tests measure and DESIGN.md quotes)"""
    import json, os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name), "a") as f:
        f.write(json.dumps(obj) + "\n")


def _assert_grad_close(got, ref, tag, tol=4e-6):
    """gradients against the reference's vectors: 4e-6 of the gradient's own scale (d/ds of the soft sort carries a factor 1/T: entries
    up to 130 at T = 2e-3, where one fp32 ulp is 8e-6).  Measured on the MI355X (profiles/r03a_grad_errors.jsonl): 9e-8 ... 3.1e-6 of
    the scale -- the largest on softsort_n16_t0.01/gm (6.7e-6 on a gradient of 2.2: the soft sort's adjoint behind the layer's, both
    fp32; the reference's own fp32 autograd is as far from an fp64 evaluation); the adjoint against an fp64 evaluation: <= 3.6e-7."""
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    _record("grad_errors.jsonl", {"what": tag, "max_abs_err": err, "scale": scale, "err_over_scale": err / scale, "tol_over_scale": tol})
    assert err <= tol * scale, f"{tag}: max |d| = {err:.3e} > {tol:g} x scale {scale:.3g}"


def test_soft_sort(G, golden_misc):
    g = golden_misc
    tags = sorted({k.split("/")[0] for k in g.keys if k.startswith("softsort_")})
    for tag in tags:
        s, m, t = g[f"{tag}/scores"], g[f"{tag}/iou"], float(g[f"{tag}/temperature"])
        ss, C, sm = G.soft_sort(torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda(), t)
        np.testing.assert_allclose(C.cpu().numpy(), g[f"{tag}/C"], atol=1e-5)
        np.testing.assert_allclose(ss.cpu().numpy(), g[f"{tag}/soft_scores"], atol=1e-5)
        np.testing.assert_allclose(sm.cpu().numpy(), g[f"{tag}/soft_matrix"], atol=1e-5)
        for mt, kw in (("gm", dict(group_boxes=True, mask_group_boxes=True)),
                       ("gu", dict(group_boxes=True, mask_group_boxes=False)), ("un", dict(group_boxes=False))):
            res = _run_gpu(G, s, m, g[f"{tag}/w"], True, sorting_method="soft", sorting_temperature=t, temperature=0.1, **kw)
            np.testing.assert_allclose(res["prob"], g[f"{tag}/{mt}/prob"], atol=TOL, err_msg=f"{tag}/{mt}")
            check_index_lists(res["valid"], res["invalid"], g[f"{tag}/{mt}/valid"], g[f"{tag}/{mt}/invalid"])
            # gradients: 1e-4 (north_star) in units of the gradient's own scale -- d/ds carries a factor 1/T (T = 2e-3 .. 1e-2: entries up
            # to 130), where one fp32 ulp is already 8e-6; measured against these vectors: <= 3e-5 absolute, i.e. 2e-7 of the scale
            _assert_grad_close(res["grad_scores"], g[f"{tag}/{mt}/grad_scores"], f"{tag}/{mt} grad_scores")
            _assert_grad_close(res["grad_iou"], g[f"{tag}/{mt}/grad_iou"], f"{tag}/{mt} grad_iou")


def test_sgemm_mfma(G):
    from groomed_nms_amd.groomed_nms import _sgemm
    rng = np.random.default_rng(0)
    # (the last four: the 256 x 128 kernel -- one slice of K at 4096 x 2048, split K below that: 4 x 2 tiles x 16 / 8, 8 x 8 x 4 slices)
    for M, N, K in ((1, 1, 1), (33, 65, 17), (128, 128, 128), (200, 300, 250), (512, 384, 1024), (1024, 1024, 1024), (512, 256, 2048), (2048, 1024, 512),
                    (4096, 2048, 64)):
        a = rng.uniform(-1, 1, size=(M, K)).astype(np.float32)
        b = rng.uniform(-1, 1, size=(K, N)).astype(np.float32)     # asymmetric operands
        got = _sgemm(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        ref = a.astype(np.float64) @ b.astype(np.float64)
        np.testing.assert_allclose(got, ref, atol=1e-6 * K + 1e-5, rtol=1e-5)


@pytest.mark.gpu
def test_sgemm_every_path_against_float64(G):
    """Round 6: the plain product behind the soft sort goes to rocBLAS from 512^3 on and to hipBLASLt from 2048^3 on (dlopen at first use),
    the library's own MFMA kernels serve everything else; gnms_profile_sgemm selects a path.  Every path against the float64 product on
    asymmetric operands, row-major with padded leading dimensions (the column-major trick D^T = B^T A^T must not transpose anything), shapes on
    both sides of the dispatch's thresholds; a path whose library is missing may refuse (GNMS_ERR_UNSUPPORTED), never return a wrong product."""
    import ctypes
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    dev = torch.device("cuda")
    rng = np.random.default_rng(5)
    for M, N, K, pad in ((300, 500, 700, 0), (512, 512, 512, 4), (640, 2048, 1024, 8), (2048, 2304, 2048, 0), (2560, 2048, 2176, 16)):
        a = rng.uniform(-1, 1, size=(M, K + pad)).astype(np.float32)
        b = rng.uniform(-1, 1, size=(K, N + pad)).astype(np.float32)
        ref = a[:, :K].astype(np.float64) @ b[:, :N].astype(np.float64)
        at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        for variant in (0, 1, 2, 3, 4):
            d = torch.full((M, N + pad), -7.0, device=dev)
            rc = lib.gnms_profile_sgemm(ptr(at), ptr(bt), ptr(d), M, N, K, K + pad, N + pad, N + pad, variant, stream_ptr(dev))
            if rc == -2 and variant in (2, 4):            # GNMS_ERR_UNSUPPORTED: the vendor library is not in this process / image
                continue
            assert rc == 0, (M, N, K, variant, lib.gnms_last_error())
            got = d.cpu().numpy()
            np.testing.assert_allclose(got[:, :N], ref, atol=1e-6 * K + 1e-5, rtol=1e-5, err_msg=str((M, N, K, variant)))
            if pad:
                assert np.all(got[:, N:] == -7.0), (M, N, K, variant)     # the padding columns of D stay untouched


def test_classic_nms(G, O, golden_misc):
    from groomed_nms_amd.nms import gpu_nms
    g = golden_misc
    for tag in ("dets40", "dets300", "dets_uni200"):
        dets = g[f"{tag}/dets"]
        for thr in (0.4, 0.7):
            got = [int(i) for i in gpu_nms(dets, thr, device_id=0)]
            assert got == list(g[f"{tag}/py_cpu_nms_{thr}"]), (tag, thr)
            assert got == O.classic_nms(dets, thr, rule="gpu")
    assert gpu_nms(np.zeros((0, 5), np.float32), 0.4) == []
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 1000, 4096):
        dets = np.concatenate([synthetic.clustered_boxes_2d(rng, n, 16), synthetic.tie_free_scores(rng, n)[:, None]], 1)
        assert [int(i) for i in gpu_nms(dets, 0.5)] == O.classic_nms(dets, 0.5, rule="gpu"), n


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 257, 1000, 1024])
def test_random_vs_oracle(G, O, n):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(100 + n)
    for kind in ("uniform", "clustered"):
        b = synthetic.uniform_boxes_2d(rng, n) if kind == "uniform" else synthetic.clustered_boxes_2d(rng, n, 32)
        s = synthetic.tie_free_scores(rng, n)
        m = O.iou2d(b, b)
        w = rng.uniform(-1, 2, size=n).astype(np.float32)
        for mode in ("gm_lin", "gm_lin_gs2", "gm_sig", "gm_lin_sorted", "gu_lin", "gu_soft", "un_lin", "un_sig"):
            if n > 300 and mode.startswith("un"):
                continue
            res = _run_gpu(G, s, m, w, n <= 130, **MODES[mode])
            ref = O.differentiable_nms(s, m, grad_prob=w, want_grad_iou=(n <= 130), **MODES[mode])
            tag = f"n={n} {kind} {mode}"
            if mode.startswith("gm_lin"):
                assert np.array_equal(res["prob"], ref["prob"]), tag
                assert np.array_equal(res["grad_scores"], ref["grad_scores"]), tag
                assert list(res["valid"]) == list(ref["valid"]) and list(res["invalid"]) == list(ref["invalid"]), tag
            else:
                np.testing.assert_allclose(res["prob"], ref["prob"], atol=TOL, err_msg=tag)
                np.testing.assert_allclose(res["grad_scores"], ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=tag)
                check_index_lists(res["valid"], res["invalid"], ref["valid"], ref["invalid"])
            if n <= 130:
                np.testing.assert_allclose(res["grad_iou"], ref["grad_iou"], atol=5e-4, rtol=1e-3, err_msg=tag)


def test_batched_ragged(G, O):
    """Padded batch with per-image counts (ragged inputs), including an empty image."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(7)
    B, N = 5, 200
    counts = np.array([200, 0, 1, 77, 130], np.int32)
    boxes = np.stack([synthetic.clustered_boxes_2d(rng, N, 16) for _ in range(B)])
    scores = np.stack([synthetic.tie_free_scores(rng, N) for _ in range(B)])
    from groomed_nms_amd import overlaps
    bt = torch.from_numpy(boxes).cuda()
    iou = overlaps.iou_batched(bt)
    st = torch.from_numpy(scores).cuda().requires_grad_(True)
    prob, order, valid, invalid, nv, ni = G.differentiable_nms_batched(st, iou, counts=torch.from_numpy(counts).cuda())
    w = torch.from_numpy(rng.uniform(-1, 2, size=(B, N)).astype(np.float32)).cuda()
    (prob * w).sum().backward()
    for b in range(B):
        n = int(counts[b])
        ref = O.differentiable_nms(scores[b, :n], O.iou2d(boxes[b, :n], boxes[b, :n]), grad_prob=w[b, :n].cpu().numpy())
        assert np.array_equal(prob[b, :n].detach().cpu().numpy(), ref["prob"]), b
        assert int(nv[b]) == len(ref["valid"]) and int(ni[b]) == len(ref["invalid"])
        assert valid[b, :int(nv[b])].tolist() == list(ref["valid"])
        assert np.array_equal(st.grad[b, :n].cpu().numpy(), ref["grad_scores"]), b
        assert torch.all(st.grad[b, n:] == 0) and torch.all(prob[b, n:] == 0)


def test_full_size_properties(G):
    """BASELINE sizes (N=4096, B=8; N=16384, B=2): size-independent properties of the layer."""
    from groomed_nms_amd import synthetic, overlaps
    for B, N, kind in ((8, 4096, "clustered"), (2, 16384, "uniform")):
        boxes, scores = synthetic.batch_2d(11, B, N, kind)
        bt, st = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda().requires_grad_(True)
        iou = overlaps.iou_batched(bt)
        prob, order, valid, invalid, nv, ni = G.differentiable_nms_batched(st, iou)
        prob.sum().backward()
        p = prob.detach()
        assert torch.all((p >= 0) & (p <= 1))
        sorted_scores = torch.gather(st.detach(), 1, order)
        assert torch.all(sorted_scores[:, :-1] > sorted_scores[:, 1:])               # order is the descending argsort
        assert torch.all(p <= sorted_scores + 1e-7)                                 # rescoring never raises a score
        assert torch.all(nv + ni == N)
        for b in range(B):
            v = valid[b, :int(nv[b])]
            iv = invalid[b, :int(ni[b])]
            assert len(set(v.tolist()) | set(iv.tolist())) == N                     # a partition of the boxes
            rank_of = torch.empty(N, dtype=torch.long, device="cuda")
            rank_of[order[b]] = torch.arange(N, device="cuda")
            pv = p[b][rank_of[v]]
            assert torch.all(pv[:-1] >= pv[1:]) and torch.all(pv >= 0.3)            # valid list sorted by re-score
            assert torch.all(p[b][rank_of[iv]] < 0.3)
            # kept boxes with an unchanged score are greedy-NMS leaders: mutually non-overlapping
            lead = order[b][(p[b] == sorted_scores[b].clamp(0, 1))]
            sub = iou[b][lead][:, lead]
            sub.fill_diagonal_(0)
            assert float(sub.max()) <= 0.4 + 1e-7
        # idempotence of the sort path: feeding the already-sorted problem gives the same probabilities
        iou_sorted = torch.stack([iou[b][order[b]][:, order[b]] for b in range(B)])
        prob2 = G.differentiable_nms_batched(sorted_scores, iou_sorted)[0]
        assert torch.equal(prob2, p)
        g = st.grad
        assert torch.isfinite(g).all()


# --------------------------------------------------------------------------------------------------------------
# edge cases and larger sizes against the oracle
# --------------------------------------------------------------------------------------------------------------
def _cmp_exact(res, ref, tag):
    assert np.array_equal(res["prob"], ref["prob"], equal_nan=True), tag + " prob"
    assert list(res["valid"]) == list(ref["valid"]), tag + " valid"
    assert sorted(res["invalid"]) == sorted(ref["invalid"]), tag + " invalid"
    if "grad_scores" in res:
        assert np.array_equal(res["grad_scores"], ref["grad_scores"]), tag + " grad"


@pytest.mark.parametrize("kind", ["clustered", "uniform"])
def test_n4096_single_image_bit_exact(G, O, kind):
    """BASELINE size N=4096 against the oracle, default mode: probabilities, lists and gradient bit for bit."""
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(77, 1, 4096, kind)
    m = O.iou2d(boxes[0], boxes[0])
    w = np.linspace(-1, 2, 4096).astype(np.float32)
    res = _run_gpu(G, scores[0], m, w, False)
    ref = O.differentiable_nms(scores[0], m, grad_prob=w)
    _cmp_exact(res, ref, kind)


def test_odd_sizes_and_strided_matrix(G, O):
    """N not a multiple of 4/64 (scalar load path) and a matrix whose row stride is larger than N."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(21)
    for n in (3, 61, 67, 255, 1001):
        b = synthetic.clustered_boxes_2d(rng, n, 8)
        s = synthetic.tie_free_scores(rng, n)
        m = O.iou2d(b, b)
        w = rng.uniform(-1, 2, size=n).astype(np.float32)
        ref = O.differentiable_nms(s, m, grad_prob=w)
        _cmp_exact(_run_gpu(G, s, m, w, False), ref, f"n={n}")
        # strided view: the layer must honour ld = stride(0) without copying
        big = torch.zeros((n, n + 7), device="cuda")
        big[:, :n] = torch.from_numpy(m).cuda()
        view = big[:, :n]
        assert not view.is_contiguous()
        st = torch.from_numpy(s).cuda()
        valid, invalid, prob = G.differentiable_nms(st, view)
        assert np.array_equal(prob.cpu().numpy(), ref["prob"]) and valid.tolist() == list(ref["valid"]), f"strided n={n}"


def test_ties_are_broken_stably(G, O):
    """Duplicate scores: the build defines the order as stable (lower index first), like the oracle."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(5)
    n = 200
    b = synthetic.clustered_boxes_2d(rng, n, 8)
    s = np.round(synthetic.tie_free_scores(rng, n), 1)          # 11 distinct values -> many ties
    m = O.iou2d(b, b)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    for mode in ("gm_lin", "gm_lin_gs2", "gm_lin_sorted"):
        ref = O.differentiable_nms(s, m, grad_prob=w, **MODES[mode])
        _cmp_exact(_run_gpu(G, s, m, w, False, **MODES[mode]), ref, mode)
    order = torch.sort(torch.from_numpy(s), descending=True, stable=True)[1].numpy()
    assert list(order) == list(O.argsort_desc(s))


def test_degenerate_overlaps(G, O):
    """NaN entries: a zero-area box (NaN self-overlap, lib/core.py:507) whose group is non-empty, NaN against the leader,
    a diagonal below the threshold.  The reference raises / loops on some of these; the build and the oracle
    share one definition."""
    s = np.array([0.95, 0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    m = np.eye(6, dtype=np.float32)
    m[0, 0] = np.nan            # leader 0 does not belong to its own group ...
    m[2, 0] = 0.9               # ... but box 2 does: group [2], head = 2
    m[3, 0] = 0.8
    m[4, 1] = np.nan            # box 4 vanishes (NaN against leader 1)
    m[5, 5] = 0.2               # diagonal <= threshold: leader 5 leaves, in no group
    w = np.arange(1, 7, dtype=np.float32)
    for mode in ("gm_lin", "gu_lin"):
        ref = O.differentiable_nms(s, m, grad_prob=w, want_grad_iou=True, **MODES[mode])
        res = _run_gpu(G, s, m, w, True, **MODES[mode])
        np.testing.assert_allclose(res["prob"], ref["prob"], atol=1e-6, equal_nan=True, err_msg=mode)
        assert sorted(res["valid"]) == sorted(ref["valid"]) and sorted(res["invalid"]) == sorted(ref["invalid"]), mode
        np.testing.assert_allclose(res["grad_scores"], ref["grad_scores"], atol=1e-6, err_msg=mode)
        np.testing.assert_allclose(res["grad_iou"], ref["grad_iou"], atol=1e-6, err_msg=mode)
    assert ref["prob"][0] == 0 and ref["prob"][4] == 0 and ref["prob"][5] == 0      # the three boxes that fall out of every group


def test_parameter_extremes(G, O):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(8)
    n = 300
    b = synthetic.clustered_boxes_2d(rng, n, 150)                # two huge clusters: groups beyond every cap
    s = synthetic.tie_free_scores(rng, n)
    m = O.iou2d(b, b)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    cases = [dict(group_size=0), dict(group_size=1), dict(group_size=500), dict(nms_threshold=0.0), dict(nms_threshold=0.999),
             dict(valid_box_prob_threshold=0.0), dict(valid_box_prob_threshold=1.0),
             dict(mask_group_boxes=False, group_size=500), dict(mask_group_boxes=False, group_size=120),
             dict(mask_group_boxes=False, group_size=3), dict(group_boxes=False)]
    for kw in cases:
        ref = O.differentiable_nms(s, m, grad_prob=w, **kw)
        res = _run_gpu(G, s, m, w, False, **kw)
        np.testing.assert_allclose(res["prob"], ref["prob"], atol=TOL, err_msg=str(kw))
        check_index_lists(res["valid"], res["invalid"], ref["valid"], ref["invalid"])
        np.testing.assert_allclose(res["grad_scores"], ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=str(kw))


def test_batched_equals_per_image(G):
    from groomed_nms_amd import synthetic, overlaps
    boxes, scores = synthetic.batch_2d(3, 4, 700, "clustered", per=20)
    bt, st = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    iou = overlaps.iou_batched(bt)
    prob, order, valid, invalid, nv, ni = G.differentiable_nms_batched(st, iou)
    for b in range(4):
        v1, i1, p1 = G.differentiable_nms(st[b], iou[b])
        assert torch.equal(p1, prob[b]) and torch.equal(v1, valid[b, :int(nv[b])]) and torch.equal(i1, invalid[b, :int(ni[b])])
        assert torch.all(valid[b, int(nv[b]):] == -1) and torch.all(invalid[b, int(ni[b]):] == -1)
    empty = G.differentiable_nms_batched(torch.zeros((2, 0), device="cuda"), torch.zeros((2, 0, 0), device="cuda"))
    assert empty[0].shape == (2, 0) and int(empty[4].sum()) == 0
    v, i, p = G.differentiable_nms(torch.zeros(0, device="cuda"), torch.zeros((0, 0), device="cuda"))
    assert v.numel() == 0 and i.numel() == 0 and p.numel() == 0


def test_soft_sort_larger(G, O):
    """soft sort at a size that spans several MFMA tiles, sorted input (the only regime where the reference terminates)."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(31)
    n = 300
    b = synthetic.clustered_boxes_2d(rng, n, 6)
    s = np.sort(synthetic.tie_free_scores(rng, n))[::-1].copy()
    m = O.iou2d(b, b)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    ss, C, sm = G.soft_sort(torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda(), 2e-4)
    oss, oC, osm = O.soft_sort(s, m, 2e-4)
    np.testing.assert_allclose(C.cpu().numpy(), oC, atol=2e-5)
    np.testing.assert_allclose(sm.cpu().numpy(), osm, atol=2e-4)
    ref = O.differentiable_nms(s, m, sorting_method="soft", sorting_temperature=2e-4, grad_prob=w)
    res = _run_gpu(G, s, m, w, False, sorting_method="soft", sorting_temperature=2e-4)
    np.testing.assert_allclose(res["prob"], ref["prob"], atol=TOL)
    check_index_lists(res["valid"], res["invalid"], ref["valid"], ref["invalid"])
    _assert_grad_close(res["grad_scores"], ref["grad_scores"], "soft sort n=300 T=2e-4 (fp64 adjoint of the oracle)", tol=1e-6)
    # the adjoint through the C ABI with every upstream gradient present, rectangular matrix included
    for k in (n, 77):
        mk = np.ascontiguousarray(m[:, :k])
        st = torch.from_numpy(s).cuda().requires_grad_(True)
        mt = torch.from_numpy(mk).cuda().requires_grad_(True)
        ss_, C_, sm_ = G.soft_sort(st, mt, 0.01)
        gs_, gC_, gm_ = (torch.from_numpy(rng.uniform(-1, 1, size=x.shape).astype(np.float32)).cuda() for x in (ss_, C_, sm_))
        ((ss_ * gs_).sum() + (C_ * gC_).sum() + (sm_ * gm_).sum()).backward()
        sd = torch.from_numpy(s).cuda().double().requires_grad_(True)          # the reference's expressions (:145-164) in fp64 autograd
        md = torch.from_numpy(mk).cuda().double().requires_grad_(True)
        shat = torch.sort(sd, descending=True)[0]
        A = -(sd.unsqueeze(0) - shat.unsqueeze(1)).abs()
        E = torch.exp((A - A.max(dim=1, keepdim=True)[0]) / 0.01)
        Cd = E / (E.sum(dim=1) + 1e-3)
        ((Cd @ sd * gs_.double()).sum() + (Cd * gC_.double()).sum() + ((Cd @ md) * gm_.double()).sum()).backward()
        _assert_grad_close(st.grad.cpu().numpy(), sd.grad.float().cpu().numpy(), f"soft_sort adjoint d_scores k={k}", tol=1e-6)
        _assert_grad_close(mt.grad.cpu().numpy(), md.grad.float().cpu().numpy(), f"soft_sort adjoint d_matrix k={k}", tol=1e-6)


def test_classic_nms_wide_rows_and_device_entry(G, O):
    """`_nms` with boxes_dim > 5 (stride honoured, nms_kernel.cu reads the first five fields) and the device-pointer entry."""
    import ctypes
    from groomed_nms_amd import synthetic, _lib
    from groomed_nms_amd.nms import gpu_nms
    from groomed_nms_amd._lib import ptr, check
    rng = np.random.default_rng(2)
    n = 500
    dets5 = np.concatenate([synthetic.clustered_boxes_2d(rng, n, 10), synthetic.tie_free_scores(rng, n)[:, None]], 1).astype(np.float32)
    dets7 = np.concatenate([dets5, rng.uniform(size=(n, 2)).astype(np.float32)], 1)
    want = O.classic_nms(dets5, 0.45, rule="gpu")
    assert [int(i) for i in gpu_nms(dets7, 0.45)] == want
    lib = _lib.load()
    order = dets5[:, 4].argsort()[::-1]
    sd = torch.from_numpy(np.ascontiguousarray(dets5[order])).cuda()
    keep = torch.empty(n, dtype=torch.int32, device="cuda")
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gnms_nms_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    check(lib.gnms_nms_sorted(ptr(sd), n, 5, 0.45, ptr(keep), ptr(num), ptr(ws), ws.numel(), None), "gnms_nms_sorted")
    torch.cuda.synchronize()
    assert [int(order[i]) for i in keep[:int(num)].tolist()] == want


def test_from_boxes_path_is_bit_identical(G):
    """gnms_forward_from_boxes / gnms_backward_from_boxes (no N x N matrix) == iou_batched + the matrix path, bit for bit,
    including ragged counts, the group-size cap, unmasked groups and sorted output."""
    from groomed_nms_amd import synthetic, overlaps
    from groomed_nms_amd._lib import GnmsError
    for B, N, per in ((3, 500, 20), (2, 4096, 64), (1, 64, 8), (2, 1001, 250), (2, 300, 150)):
        boxes, scores = synthetic.batch_2d(13, B, N, "clustered", per=per)
        boxes[0, 3 % N, 2:] = boxes[0, 3 % N, :2]                 # a zero-area box: NaN self-overlap
        bt = torch.from_numpy(boxes).cuda()
        counts = torch.tensor([N] + [max(1, N // 3)] * (B - 1), dtype=torch.int32).cuda()
        w = torch.rand((B, N), device="cuda")
        for kw in (dict(), dict(group_size=2), dict(mask_group_boxes=False, group_size=40), dict(return_sorted_prob=True),
                   dict(pruning_method="sigmoidal", temperature=0.1), dict(nms_threshold=0.7, valid_box_prob_threshold=0.5)):
            s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
            s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
            out1 = G.differentiable_nms_from_boxes_batched(s1, bt, counts=counts, **kw)
            out2 = G.differentiable_nms_batched(s2, overlaps.iou_batched(bt), counts=counts, **kw)
            for a, b in zip(out1, out2):
                assert torch.equal(a, b) or (a.dtype.is_floating_point and torch.allclose(a, b, atol=0, rtol=0, equal_nan=True)), (B, N, kw)
            (out1[0] * w).sum().backward()
            (out2[0] * w).sum().backward()
            assert torch.equal(s1.grad, s2.grad), (B, N, kw)
    with pytest.raises(GnmsError):
        import ctypes
        from groomed_nms_amd.groomed_nms import _params, _LayerFunction, _MODE_BOXES
        _LayerFunction.apply(torch.rand((1, 8), device="cuda"), torch.rand((1, 8, 4), device="cuda"), None,
                             _params(0.4, "linear", 0.01, 0.3, False, False, True, 100), None, _MODE_BOXES, None)     # ungrouped needs the matrix


def test_capturable_in_a_hip_graph(G):
    """The C-ABI calls are stream-ordered with no hidden allocation or synchronisation: IoU + forward + backward captured
    once into a HIP graph (torch.cuda.CUDAGraph) and replayed on new inputs give the same result as eager calls."""
    import ctypes
    from groomed_nms_amd import synthetic, _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, check
    lib = _lib.load()
    B, N = 4, 1024
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    dev = torch.device("cuda")
    boxes = torch.empty((B, N, 4), device=dev)
    scores = torch.empty((B, N), device=dev)
    gprob = torch.empty((B, N), device=dev)
    iou = torch.empty((B, N, N), device=dev)
    prob = torch.empty((B, N), device=dev)
    gscores = torch.empty((B, N), device=dev)
    ws = torch.empty(lib.gnms_workspace_bytes(B, N, ctypes.byref(P)), dtype=torch.uint8, device=dev)

    def run(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        check(lib.gnms_iou2d(ptr(boxes), ptr(boxes), B, N, N, ptr(iou), N, sp), "iou")
        check(lib.gnms_forward(ptr(scores), ptr(iou), B, N, N, None, ctypes.byref(P), ptr(prob), None, None, None, None, None, ptr(ws),
                               ws.numel(), sp), "fwd")
        check(lib.gnms_backward(ptr(gprob), ptr(scores), ptr(iou), B, N, N, None, ctypes.byref(P), ptr(gscores), None, ptr(ws), ws.numel(),
                                sp), "bwd")

    def load(seed):
        b, s = synthetic.batch_2d(seed, B, N, "clustered", per=32)
        boxes.copy_(torch.from_numpy(b)); scores.copy_(torch.from_numpy(s))
        gprob.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-1, 2, size=(B, N)).astype(np.float32)))

    load(1)
    run(torch.cuda.current_stream())            # warm-up outside capture (sets the >64 KiB LDS attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream())
    for seed in (2, 3):
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        p_graph, g_graph = prob.clone(), gscores.clone()
        run(torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert torch.equal(p_graph, prob) and torch.equal(g_graph, gscores)
        assert float(p_graph.abs().sum()) > 0


def test_iou_and_forward_in_one_call(G):
    """gnms_forward_with_iou2d (score sort inside the IoU launch for N <= 4096, two launches above) == iou_batched +
    differentiable_nms_batched: matrix, all six outputs and the gradient bit for bit; ragged counts; repeated calls."""
    from groomed_nms_amd import synthetic, overlaps
    for B, N in ((3, 500), (8, 4096), (1, 64), (2, 1001), (200, 520), (300, 1100), (1, 5000)):      # (300 images: more chain workgroups than CUs)
        boxes, scores = synthetic.batch_2d(9, B, N, "clustered", per=32)
        bt = torch.from_numpy(boxes).cuda()
        counts = torch.tensor([N] + [max(1, N // 2)] * (B - 1), dtype=torch.int32).cuda()
        w = torch.rand((B, N), device="cuda")
        for rep in range(2):
            s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
            s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
            out1 = G.differentiable_nms_with_iou2d_batched(s1, bt, counts=counts)
            iou = overlaps.iou_batched(bt)
            out2 = G.differentiable_nms_batched(s2, iou, counts=counts)
            assert torch.equal(out1[6], iou), (B, N)
            for a, b in zip(out1[:6], out2):
                assert torch.equal(a, b), (B, N)
            (out1[0] * w).sum().backward()
            (out2[0] * w).sum().backward()
            assert torch.equal(s1.grad, s2.grad), (B, N)


# ------------------------------------------------------------------------------------------------
# the after-NMS AP loss (lib/loss/aploss.py), the consumer of the rescored scores
# ------------------------------------------------------------------------------------------------
APLOSS_TOL = 2e-5          # fp32 sums over <= 4096 terms in a different association than torch.sum


def test_aploss_against_reference_vectors():
    """APLoss/backpropAPLoss (HIP) vs vectors captured from lib/loss/aploss.py: loss, gradient after an upstream
    scale, return shapes (scalar; shape (1,) zeros when no positive), CPU-in/CPU-out."""
    from conftest import Golden
    from groomed_nms_amd.aploss import APLoss
    g = Golden("aploss.npz")
    crit = APLoss()
    for tag in g.cases():
        lg = torch.from_numpy(g[f"{tag}/logits"]).cuda().requires_grad_(True)
        tg = torch.from_numpy(g[f"{tag}/targets"]).cuda()
        loss = crit(lg, tg)
        want = g[f"{tag}/loss"]
        if tag == "nopos":
            assert loss.shape == (1,) and float(loss.detach()) == 0.0
        else:
            assert loss.dim() == 0, tag
        np.testing.assert_allclose(loss.detach().cpu().numpy().reshape(-1), want.reshape(-1), atol=APLOSS_TOL, err_msg=tag)
        up = float(g[f"{tag}/upstream"])
        (loss.sum() * up).backward()
        np.testing.assert_allclose(lg.grad.cpu().numpy(), g[f"{tag}/grad"], atol=APLOSS_TOL, rtol=1e-4, err_msg=tag)
    # CPU tensors in -> CPU tensors out (the reference runs wherever its inputs live, aploss.py:21-24)
    lg = torch.from_numpy(g["u50_10/logits"]).requires_grad_(True)
    loss = crit(lg, torch.from_numpy(g["u50_10/targets"]))
    assert not loss.is_cuda
    loss.backward()
    assert not lg.grad.is_cuda
    np.testing.assert_allclose(lg.grad.numpy() * float(g["u50_10/upstream"]), g["u50_10/grad"], atol=APLOSS_TOL, rtol=1e-4)


def test_aploss_against_oracle_random():
    """Seeded cases up to the 4096-box limit against the C oracle: wide logits (saturating ranks), ties, labels other
    than 0/1 ignored, ragged counts and the `active` mask of the batched entry; one launch for the whole batch."""
    import oracle.oracle as O
    from groomed_nms_amd.aploss import ap_loss_batched
    rng = np.random.default_rng(5)
    for B, N, spread, npos in ((4, 500, 1.0, 20), (3, 4096, 1.0, 300), (2, 1000, 6.0, 64), (5, 37, 0.2, 5), (2, 2048, 3.0, 1500)):
        lg = (rng.standard_normal((B, N)) * spread).astype(np.float32)
        if spread < 1:
            lg = np.round(lg * 8) / 8                                    # ties
        tg = np.zeros((B, N), np.float32)
        for b in range(B):
            tg[b, rng.choice(N, size=min(npos, N), replace=False)] = 1
            tg[b, rng.choice(N, size=N // 10, replace=False)] = -1      # "ignore" labels (neither positive nor negative)
        tg[B - 1, :] = np.where(tg[B - 1] == 1, 0, tg[B - 1]) if B > 3 else tg[B - 1]   # one image without positives
        counts = np.array([N] + [max(1, (N * 2) // 3)] * (B - 1), np.int32)
        active = rng.uniform(size=(B, N)) < 0.8
        for use_counts, use_active in ((False, False), (True, False), (False, True)):
            lt = torch.from_numpy(lg).cuda().requires_grad_(True)
            loss = ap_loss_batched(lt, torch.from_numpy(tg).cuda(),
                                   active=torch.from_numpy(active).cuda() if use_active else None,
                                   counts=torch.from_numpy(counts).cuda() if use_counts else None)
            w = torch.arange(1, B + 1, device="cuda", dtype=torch.float32)
            (loss * w).sum().backward()
            for b in range(B):
                n = int(counts[b]) if use_counts else N
                sel = active[b, :n] if use_active else np.ones(n, bool)
                ol, og = O.aploss(lg[b, :n][sel], tg[b, :n][sel])
                assert abs(float(loss[b].detach()) - ol) <= APLOSS_TOL, (B, N, b, use_counts, use_active)
                want = np.zeros(N, np.float32)
                want[:n][sel] = og * (b + 1)
                np.testing.assert_allclose(lt.grad[b].cpu().numpy(), want, atol=APLOSS_TOL, rtol=2e-4,
                                           err_msg=str((B, N, b, use_counts, use_active)))


def test_aploss_properties_and_limits():
    """Size-independent properties at the limit: perfectly separated scores give loss 0, inverted ones the known
    closed form, the gradient sums to ~0 over positives+negatives weights..., N above the limit raises."""
    from groomed_nms_amd import _lib
    from groomed_nms_amd.aploss import ap_loss_batched
    N, F = 4096, 128
    tg = torch.zeros((2, N), device="cuda")
    tg[:, :F] = 1
    lg = torch.empty((2, N), device="cuda")
    lg[0, :F] = 10.0; lg[0, F:] = -10.0                    # all positives above all negatives by > delta: AP = 1
    lg[1, :F] = -10.0; lg[1, F:] = 10.0                    # all positives below every negative
    lg = lg.requires_grad_(True)
    loss = ap_loss_batched(lg, tg)
    assert abs(float(loss[0].detach())) < 1e-6
    # inverted: each positive has rank a = 0.5*(F-1)+1 among positives (equal logits -> 0.5 each, +0.5 self +0.5), b = N-F
    a = 0.5 * (F - 1) + 1.0
    assert abs(float(loss[1]) - (1 - a / (a + (N - F)))) < 1e-5
    loss.sum().backward()
    assert float(lg.grad[0].abs().max()) == 0.0 or float(loss[0]) < 1e-6
    assert torch.isfinite(lg.grad).all()
    # positives are pushed up, negatives down
    assert (lg.grad[1, :F] < 0).all() and (lg.grad[1, F:] >= 0).all()
    with pytest.raises(_lib.GnmsError):
        ap_loss_batched(torch.zeros((1, 20000), device="cuda"), torch.zeros((1, 20000), device="cuda"))


def test_aploss_large_images_and_many_positives():
    """N up to GNMS_MAX_BOXES and F in the thousands (the spread version: positives over the machine) against the oracle; the
    one-workgroup version (N < 2048) and the spread version (same boxes padded to N = 2048 with a count) give the same numbers."""
    from groomed_nms_amd.aploss import ap_loss_batched
    from oracle import oracle as O
    rng = np.random.default_rng(23)
    for N, F in ((6000, 300), (16384, 2500), (4096, 1024), (2048, 1)):
        B = 2
        lg = rng.normal(0, 2.0, size=(B, N)).astype(np.float32)
        tg = np.zeros((B, N), np.float32)
        for b in range(B):
            tg[b, rng.choice(N, F, replace=False)] = 1
        tg[1, rng.choice(N, 50, replace=False)] = -1                 # ignored label
        lt = torch.from_numpy(lg).cuda().requires_grad_(True)
        loss = ap_loss_batched(lt, torch.from_numpy(tg).cuda())
        loss.sum().backward()
        for b in range(B):
            rl, rg = O.aploss(lg[b], tg[b])
            assert abs(float(loss[b]) - rl) <= APLOSS_TOL, (N, F, b)
            np.testing.assert_allclose(lt.grad[b].cpu().numpy(), rg, atol=APLOSS_TOL, rtol=1e-4, err_msg=str((N, F, b)))
    n = 2047
    lg = rng.normal(0, 2.0, size=(1, n)).astype(np.float32)
    tg = (rng.uniform(size=(1, n)) < 0.1).astype(np.float32)
    a = torch.from_numpy(lg).cuda().requires_grad_(True)
    la = ap_loss_batched(a, torch.from_numpy(tg).cuda())
    la.sum().backward()
    pad = torch.zeros((1, 2048), device="cuda"); pad[:, :n] = torch.from_numpy(lg).cuda()
    padt = torch.zeros((1, 2048), device="cuda"); padt[:, :n] = torch.from_numpy(tg).cuda()
    pb = pad.clone().requires_grad_(True)
    lb = ap_loss_batched(pb, padt, counts=torch.tensor([n], dtype=torch.int32))
    lb.sum().backward()
    assert abs(float(la) - float(lb)) <= 1e-6
    np.testing.assert_allclose(a.grad.cpu().numpy()[0], pb.grad.cpu().numpy()[0, :n], atol=1e-7, rtol=1e-6)
    assert float(pb.grad[0, n:].abs().max()) == 0.0


def test_from_boxes_decisions_on_adversarial_boxes(G):
    """The from-boxes bit matrix decides pairs without the division and skips rows that cannot touch a column tile's hull;
    both shortcuts must give the matrix path's bits on degenerate input: zero-area / inverted / NaN / infinite boxes,
    duplicates (IoU exactly 1), boxes that only touch, IoU values within an ulp of the threshold, thresholds 0, 1 and
    negative, everything in one column of the image (no culling possible) and everything spread out (all culled)."""
    from groomed_nms_amd import overlaps
    rng = np.random.default_rng(77)
    N = 700

    def grid_boxes(step):                       # touching / overlapping-by-a-hair neighbours
        i = np.arange(N)
        x = (i % 40) * step
        y = (i // 40) * step
        return np.stack([x, y, x + 10, y + 10], 1).astype(np.float32)

    cases = {}
    b = rng.uniform(0, 100, (N, 4)).astype(np.float32); b[:, 2:] += b[:, :2]
    b[5] = [10, 10, 10, 30]; b[6] = [50, 50, 40, 40]; b[7] = [np.nan, 0, 5, 5]; b[8] = [0, 0, np.inf, 5]
    b[9] = [-np.inf, -np.inf, np.inf, np.inf]; b[10:20] = b[20]                       # degenerate + duplicates
    cases["degenerate"] = b
    cases["touching"] = grid_boxes(10.0)
    cases["hair"] = grid_boxes(9.999999)
    tall = rng.uniform(0, 5, (N, 4)).astype(np.float32); tall[:, 1] = rng.uniform(0, 3000, N); tall[:, 2] = tall[:, 0] + 50
    tall[:, 3] = tall[:, 1] + rng.uniform(20, 90, N).astype(np.float32)
    cases["one_column"] = tall
    far = np.zeros((N, 4), np.float32); far[:, 0] = np.arange(N) * 100; far[:, 2] = far[:, 0] + 30; far[:, 3] = 30
    cases["spread"] = far
    # pairs whose IoU sits right at the threshold: box k = [0, 0, 10, h_k] against [0, 0, 10, 10] has IoU h_k/10 (h_k < 10)
    at = np.zeros((N, 4), np.float32); at[:, 2] = 10
    at[:, 3] = np.nextafter(np.float32(4.0), np.float32(5.0)) + (np.arange(N) - N // 2).astype(np.float32) * np.float32(4.8e-7)
    at[0, 3] = 10
    cases["at_threshold"] = at
    for name, bx in cases.items():
        sc = rng.permutation(N).astype(np.float32) / N
        bt = torch.from_numpy(np.stack([bx, bx[::-1].copy()])).cuda()
        st = torch.from_numpy(np.stack([sc, sc])).cuda()
        iou = overlaps.iou_batched(bt)
        for thr in (0.4, 0.0, 1.0, -0.5, 0.39999998):
            out1 = G.differentiable_nms_from_boxes_batched(st, bt, nms_threshold=thr)
            out2 = G.differentiable_nms_batched(st, iou, nms_threshold=thr)
            out3 = G.differentiable_nms_with_iou2d_batched(st, bt, nms_threshold=thr)
            for a, b2, c in zip(out1, out2, out3):
                assert torch.equal(a, b2) or torch.allclose(a, b2, atol=0, rtol=0, equal_nan=True), (name, thr)
                assert torch.equal(c, b2) or torch.allclose(c, b2, atol=0, rtol=0, equal_nan=True), (name, thr)


# ------------------------------------------------------------------------------------------------
# decode + projected boxes + score top-K in front of the layer
# ------------------------------------------------------------------------------------------------
def test_proposals_against_reference_vectors_and_oracle():
    """bbox_transform_inv / projected_boxes_2d / select_topk (HIP) vs the reference's vectors and the NumPy oracle; then the
    whole front end chained into the layer: decode -> top-K (gathered, padded) -> gnms_forward_with_iou2d with counts."""
    from conftest import Golden
    import oracle.proposals_oracle as PO
    import oracle.oracle as O
    from groomed_nms_amd import proposals as PR
    import groomed_nms_amd as G
    g = Golden("proposals.npz")
    # decode: expf differs from libm by an ulp -> relative 1e-6 on widths of a few hundred pixels
    for tag in ("d2_64", "d3_3x500", "d3_1x7"):
        a = torch.from_numpy(g[f"decode/{tag}/anchors"]).cuda()
        d = torch.from_numpy(g[f"decode/{tag}/deltas"]).cuda()
        keep = d.clone()
        out = PR.bbox_transform_inv(a, d)
        assert out.shape == d.shape and torch.equal(d, keep)
        np.testing.assert_allclose(out.cpu().numpy(), g[f"decode/{tag}/out_plain"], rtol=2e-6, atol=2e-4, err_msg=tag)
        out = PR.bbox_transform_inv(a, d, means=g[f"decode/{tag}/means"], stds=g[f"decode/{tag}/stds"])
        np.testing.assert_allclose(out.cpu().numpy(), g[f"decode/{tag}/out_norm"], rtol=2e-6, atol=2e-4, err_msg=tag)
        cpu = PR.bbox_transform_inv(torch.from_numpy(g[f"decode/{tag}/anchors"]), torch.from_numpy(g[f"decode/{tag}/deltas"]))
        assert not cpu.is_cuda and cpu.shape == d.shape                      # CPU in -> CPU out, like the reference
    assert PR.bbox_transform_inv(torch.zeros((0, 4)), torch.zeros((0, 4))).shape == (0, 4)      # lib/rpn_util.py:881-882
    # projection (sinf/cosf + a 4-term dot product in another association than torch.matmul): 1e-4 relative, 5e-3 px
    for tag in ("p64", "p500"):
        par = torch.from_numpy(g[f"project/{tag}/params"]).cuda().unsqueeze(0).repeat(2, 1, 1)
        out = PR.projected_boxes_2d(par, g[f"project/{tag}/p2"], float(g[f"project/{tag}/scale"]))
        for b in range(2):
            np.testing.assert_allclose(out[b].cpu().numpy(), g[f"project/{tag}/boxes"], rtol=1e-4, atol=5e-3, err_msg=tag)
    # selection: bit-exact indices, padding, ragged candidate lists, all-boxes mode, ties keep candidate order
    for tag in ("t2000_700_500", "t2000_120_500", "t300_300_50"):
        sc, fg, K = g[f"topk/{tag}/scores"], g[f"topk/{tag}/fg"], int(g[f"topk/{tag}/K"])
        boxes = np.random.default_rng(1).uniform(0, 100, (len(sc), 4)).astype(np.float32)
        F = len(fg)
        cand = np.zeros((2, F), np.int32); cand[0] = fg; cand[1, :F // 2] = fg[::2][:F // 2]
        cnt = np.array([F, F // 2], np.int32)
        idx, num, ssel, bsel = PR.select_topk(torch.from_numpy(np.stack([sc, sc])).cuda(), K, torch.from_numpy(cand).cuda(),
                                              torch.from_numpy(cnt).cuda(), torch.from_numpy(np.stack([boxes, boxes])).cuda())
        want0 = g[f"topk/{tag}/selected"]
        want1 = PO.select_topk(sc, cand[1, :F // 2], K)
        for b, want in ((0, want0), (1, want1)):
            m = len(want)
            assert int(num[b]) == m
            assert np.array_equal(idx[b, :m].cpu().numpy(), want) and (idx[b, m:] == -1).all()
            assert np.array_equal(ssel[b, :m].cpu().numpy(), sc[want]) and (ssel[b, m:] == 0).all()
            assert np.array_equal(bsel[b, :m].cpu().numpy(), boxes[want]) and (bsel[b, m:] == 0).all()
    sc = np.round(np.random.default_rng(3).uniform(0, 1, (1, 5000)), 2).astype(np.float32)       # heavy ties, no candidate list
    idx, num, ssel, _ = PR.select_topk(torch.from_numpy(sc).cuda(), 600)
    assert int(num[0]) == 600 and np.array_equal(idx[0].cpu().numpy(), O.argsort_desc(sc[0])[:600])
    # chained: decode -> top-K -> one-call layer on the padded selection == oracle on the compacted selection
    tag = "d3_3x500"
    a = torch.from_numpy(g[f"decode/{tag}/anchors"]).cuda()
    d = torch.from_numpy(g[f"decode/{tag}/deltas"]).cuda()
    boxes = PR.bbox_transform_inv(a, d, means=g[f"decode/{tag}/means"], stds=g[f"decode/{tag}/stds"])
    rng = np.random.default_rng(9)
    scores = torch.from_numpy(rng.permutation(3 * 500).reshape(3, 500).astype(np.float32) / 1500).cuda()
    fgc = np.array([500, 220, 3], np.int32)
    cand = np.stack([rng.permutation(500) for _ in range(3)]).astype(np.int32)
    idx, num, ssel, bsel = PR.select_topk(scores, 256, torch.from_numpy(cand).cuda(), torch.from_numpy(fgc).cuda(), boxes)
    out = G.differentiable_nms_with_iou2d_batched(ssel, bsel, counts=num)
    for b in range(3):
        m = int(num[b])
        ref = O.differentiable_nms(ssel[b, :m].cpu().numpy(), O.iou2d(bsel[b, :m].cpu().numpy(), bsel[b, :m].cpu().numpy()))
        np.testing.assert_allclose(out[0][b, :m].cpu().numpy(), ref["prob"], atol=TOL)


def test_training_step_chain_against_oracle(G, O):
    """What lib/loss/rpn_3d.py does per step at its own sizes (:740-793, :1117-1131), on the GPU end to end: top-K selection ->
    overlaps + GrooMeD-NMS in one call -> after-NMS AP loss on the rescored probabilities -> backward to the raw scores.  Loss and
    dL/dscores against the same chain of oracle pieces (the ranking loss sums thousands of sigmoid-free step terms: APLOSS_TOL)."""
    from groomed_nms_amd import proposals as PR, synthetic
    from groomed_nms_amd.aploss import ap_loss_batched
    import oracle.proposals_oracle as PO
    rng = np.random.default_rng(17)
    B, A, K = 4, 1500, 500
    boxes_np, scores_np = synthetic.batch_2d(17, B, A, "clustered", per=24)
    fg_counts = np.array([A, 900, 400, 37], np.int32)                       # the last two images have fewer candidates than K
    cand = np.stack([rng.permutation(A) for _ in range(B)]).astype(np.int32)
    labels_all = (rng.uniform(size=(B, A)) < 0.08).astype(np.float32)       # label of every anchor; gathered along with the selection
    scores = torch.from_numpy(scores_np).cuda().requires_grad_(True)
    boxes = torch.from_numpy(boxes_np).cuda()
    idx, num, ssel, bsel = PR.select_topk(scores.detach(), K, torch.from_numpy(cand).cuda(), torch.from_numpy(fg_counts).cuda(), boxes)
    safe = idx.clamp(min=0).long()
    s_sel = torch.gather(scores, 1, safe) * (idx >= 0)                      # differentiable gather of the selected scores
    out = G.differentiable_nms_with_iou2d_batched(s_sel, bsel, counts=num)
    prob, order = out[0], out[1]
    # the loss ranks the rescored probabilities; their targets follow the layer's order (prob is in sorted-rank order)
    lab_sel = torch.gather(torch.from_numpy(labels_all).cuda(), 1, safe)
    lab_rank = torch.gather(lab_sel, 1, order.clamp(min=0))
    loss = ap_loss_batched(prob, lab_rank, counts=num)
    wl = torch.tensor([1.0, 0.5, 2.0, 1.5], device="cuda")
    (loss * wl).sum().backward()
    for b in range(B):
        m = int(num[b])
        sel = PO.select_topk(scores_np[b], cand[b, :fg_counts[b]], K)
        assert np.array_equal(idx[b, :m].cpu().numpy(), sel)
        sb, bb = scores_np[b][sel], boxes_np[b][sel]
        fwd = O.differentiable_nms(sb, O.iou2d(bb, bb))
        lab = labels_all[b][sel][fwd["order"]]
        ol, og = O.aploss(fwd["prob"], lab)
        assert abs(float(loss[b].detach()) - ol) <= APLOSS_TOL, b
        bwd = O.differentiable_nms(sb, O.iou2d(bb, bb), grad_prob=og * float(wl[b]))
        want = np.zeros(A, np.float32)
        want[sel] = bwd["grad_scores"]
        np.testing.assert_allclose(scores.grad[b].cpu().numpy(), want, atol=2 * APLOSS_TOL, rtol=2e-4, err_msg=str(b))


def test_fuzz_layer_against_oracle(G, O):
    """Seeded fuzz over sizes, box statistics, thresholds, group sizes, pruning functions and ragged counts: the one-call entry
    (from-boxes kernels, fused tail for small N), the matrix-in entry and the oracle must agree on every image -- probabilities
    and gradients within TOL (bit-exact between the two HIP paths), valid / invalid as sets."""
    from groomed_nms_amd import synthetic, overlaps
    rng = np.random.default_rng(20260928)
    for trial in range(120):
        B = int(rng.integers(1, 5))
        N = int(rng.choice([1, 2, 7, 63, 64, 65, 130, 257, 300, 520, 1025, 2300]))
        kind = "clustered" if rng.uniform() < 0.7 else "uniform"
        per = int(rng.choice([2, 8, 40, 150]))
        boxes, scores = synthetic.batch_2d(int(rng.integers(1 << 30)), B, N, kind, per=per)
        if rng.uniform() < 0.3:
            boxes = np.round(boxes / 8) * 8                                    # exact duplicates and exactly touching boxes
        kw = dict(nms_threshold=float(rng.choice([0.2, 0.4, 0.55, 0.75])), group_size=int(rng.choice([0, 1, 3, 100])),
                  valid_box_prob_threshold=float(rng.choice([0.0, 0.3, 0.6])),
                  return_sorted_prob=bool(rng.uniform() < 0.2))
        pm = rng.choice(["linear", "linear", "sigmoidal", "soft_nms"])
        kw.update(pruning_method=str(pm), temperature=0.01 if pm == "linear" else 0.3)
        mask = bool(rng.uniform() < 0.8)
        counts_np = np.array([N] + [int(rng.integers(1, N + 1)) for _ in range(B - 1)], np.int32)
        counts = torch.from_numpy(counts_np).cuda()
        bt = torch.from_numpy(boxes).cuda()
        w = torch.from_numpy(rng.uniform(-1, 2, (B, N)).astype(np.float32)).cuda()
        s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
        s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
        out1 = G.differentiable_nms_with_iou2d_batched(s1, bt, counts=counts, mask_group_boxes=mask, **kw)
        out2 = G.differentiable_nms_batched(s2, overlaps.iou_batched(bt), counts=counts, mask_group_boxes=mask, **kw)
        tag = (trial, B, N, kind, per, kw, mask)
        for a, b2 in zip(out1[:6], out2):
            assert torch.equal(a, b2) or torch.allclose(a, b2, atol=0, rtol=0, equal_nan=True), tag
        (out1[0] * w).sum().backward()
        (out2[0] * w).sum().backward()
        assert torch.equal(s1.grad, s2.grad), tag
        for b in range(B):
            n = int(counts_np[b])
            ref = O.differentiable_nms(scores[b, :n], O.iou2d(boxes[b, :n], boxes[b, :n]), grad_prob=w[b, :n].cpu().numpy(),
                                       mask_group_boxes=mask, **kw)
            if np.isnan(ref["prob"]).any():
                continue                                                       # zero-area duplicates: NaN self-overlap, order undefined
            np.testing.assert_allclose(out1[0][b, :n].detach().cpu().numpy(), ref["prob"], atol=TOL, err_msg=str(tag))
            np.testing.assert_allclose(s1.grad[b, :n].cpu().numpy(), ref["grad_scores"], atol=TOL, rtol=1e-4, err_msg=str(tag))
            if not kw["return_sorted_prob"]:
                nv, ni = int(out1[4][b]), int(out1[5][b])
                check_index_lists(out1[2][b, :nv].cpu().numpy(), out1[3][b, :ni].cpu().numpy(), ref["valid"], ref["invalid"])


def test_best_targets_against_reference_vectors_and_oracle():
    """SURVEY 8-f3 (lib/loss/rpn_3d.py:801-825): gnms_best_targets vs the reference's vectors and the oracle; ragged counts, a
    ground truth nobody overlaps (index -1), two ground truths choosing the same box, first-index ties."""
    from conftest import Golden
    import oracle.proposals_oracle as PO
    from groomed_nms_amd import proposals as PR
    g = Golden("proposals.npz")
    for tag in ("b300_6", "b500_1", "b40_12"):
        pp, pb = g[f"best/{tag}/pred_params"], g[f"best/{tag}/pred_boxes"]
        gp, gb = g[f"best/{tag}/gt_params"], g[f"best/{tag}/gt_boxes"]
        beta = float(g[f"best/{tag}/beta"])
        n, m = len(pp), len(gp)
        # image 0: the golden case; image 1: ragged (first half of the predictions, all but the last ground truth)
        P = torch.from_numpy(np.stack([pp, pp])).cuda(); PB = torch.from_numpy(np.stack([pb, pb])).cuda()
        Gp = torch.from_numpy(np.stack([gp, gp])).cuda(); GB = torch.from_numpy(np.stack([gb, gb])).cuda()
        pc = torch.tensor([n, max(1, n // 2)], dtype=torch.int32).cuda(); gc = torch.tensor([m, max(1, m - 1)], dtype=torch.int32).cuda()
        tg, idx, sc = PR.best_targets(P, PB, Gp, GB, beta, pc, gc)
        assert np.array_equal(tg[0].cpu().numpy(), g[f"best/{tag}/targets"]), tag
        np.testing.assert_allclose(sc[0].cpu().numpy(), g[f"best/{tag}/scores_with_gt"].max(0), atol=TOL)
        n1, m1 = max(1, n // 2), max(1, m - 1)
        otg, oidx, osc = PO.best_targets(pp[:n1], pb[:n1], gp[:m1], gb[:m1], beta)
        assert np.array_equal(tg[1, :n1].cpu().numpy(), otg) and not tg[1, n1:].any()
        assert np.array_equal(idx[1, :m1].cpu().numpy(), oidx) and (idx[1, m1:] == -1).all()
        np.testing.assert_allclose(sc[1, :m1].cpu().numpy(), osc, atol=TOL)
    # far-away ground truth -> no target; duplicate predictions -> the first one wins; two ground truths sharing the best box
    pp = np.array([[0, 1, 20, 1.6, 1.5, 4, 0.1]] * 3 + [[10, 1, 30, 1.6, 1.5, 4, 0.0]], np.float32)
    pb = np.array([[100, 100, 200, 180]] * 3 + [[400, 100, 480, 170]], np.float32)
    gp = np.array([[0, 1, 20, 1.6, 1.5, 4, 0.1], [0.1, 1, 20.2, 1.6, 1.5, 4, 0.1], [-40, 1, 80, 1.6, 1.5, 4, 0.0]], np.float32)
    gb = np.array([[100, 100, 200, 180], [102, 100, 203, 181], [900, 300, 950, 340]], np.float32)
    tg, idx, sc = PR.best_targets(*(torch.from_numpy(a).cuda().unsqueeze(0) for a in (pp, pb, gp, gb)), 0.3)
    assert idx[0].tolist() == [0, 0, -1] and tg[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert abs(float(sc[0, 0]) - 1.0) < 1e-6 and float(sc[0, 2]) == 0.0


def test_iou3d_and_forward_in_one_call(G):
    """gnms_forward_with_iou3d (threshold bits from the cuboid records, same instruction sequence as the matrix kernel) ==
    iou3d_batched(from_params, nms_overlap) + differentiable_nms_batched: the matrix, all six outputs and the gradient bit for
    bit; ragged counts, small and large N, every mode (the non-default ones read the matrix they wrote)."""
    from groomed_nms_amd import synthetic, overlaps
    for B, N, kw in ((3, 500, {}), (2, 4096, {}), (1, 64, {}), (2, 1001, dict(nms_threshold=0.6)), (2, 2300, dict(group_size=3)),
                     (2, 900, dict(nms_threshold=0.5)), (2, 900, dict(nms_threshold=0.005)), (2, 900, dict(nms_threshold=0.2)),
                     (8, 8192, {}),
                     (2, 300, dict(mask_group_boxes=False)), (1, 200, dict(group_boxes=False)), (2, 700, dict(return_sorted_prob=True))):
        par, scores = synthetic.batch_3d(11, B, N, clustered=True, per=16)
        pt = torch.from_numpy(par).cuda()
        counts = torch.tensor([N] + [max(1, N // 2)] * (B - 1), dtype=torch.int32).cuda()
        w = torch.rand((B, N), device="cuda")
        s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
        s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
        out1 = G.differentiable_nms_with_iou3d_batched(s1, pt, counts=counts, **kw)
        ov = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True, nms_threshold=kw.get("nms_threshold", 0.4))
        out2 = G.differentiable_nms_batched(s2, ov, counts=counts, **kw)
        assert torch.equal(out1[6], ov), (B, N, kw)
        for a, b in zip(out1[:6], out2):
            assert torch.equal(a, b) or torch.allclose(a, b, atol=0, rtol=0, equal_nan=True), (B, N, kw)
        (out1[0] * w).sum().backward()
        (out2[0] * w).sum().backward()
        assert torch.equal(s1.grad, s2.grad), (B, N, kw)


def _oracle_overlap3d(O, corners):
    """The reference's NMS overlap 0.5 * (1 + GIoU3D) (lib/core.py:305-421 generalized + lib/loss/rpn_3d.py:781) on the CPU."""
    return (np.float32(0.5) * (np.float32(1.0) + O.iou3d_approximate(corners, corners, generalized=True)[1])).astype(np.float32)


@pytest.mark.parametrize("B,N,clustered", [(2, 4096, True), (2, 4096, False), (1, 16384, True), (1, 16384, False)])
def test_iou3d_one_call_against_oracle_at_scale(G, O, B, N, clustered):
    """The PRODUCTION 3D path (gnms_forward_with_iou3d: re-associated overlap kernel + threshold bits from the records) against
    the CPU oracle at BASELINE sizes.  The oracle thresholds the reference's exact-order matrix; the GPU decides every pair inside
    the guard band with that same order, so the index lists must be EQUAL and the probabilities / gradients within 1e-4
    (north_star) -- measured: the matrix differs by <= 2e-6, the probabilities by <= 2e-6 * score.
    The corners come from the GPU's own get_corners_of_cuboid (sinf/cosf differ from libm by an ulp, lib/math_3d.py:364-435 is
    checked separately at 2e-5), so that the overlap arithmetic itself is compared bit for bit."""
    from groomed_nms_amd import synthetic, overlaps
    par, scores = synthetic.batch_3d(31 + N + int(clustered), B, N, clustered=clustered, per=64)
    pt = torch.from_numpy(par).cuda()
    st = torch.from_numpy(scores).cuda().requires_grad_(True)
    w = np.linspace(-1, 2, N).astype(np.float32)
    out = G.differentiable_nms_with_iou3d_batched(st, pt)
    (out[0] * torch.from_numpy(w).cuda()).sum().backward()
    exact_gpu = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True)        # exact-order kernel (iou3d_kernel<METHOD 2>)
    raw_diff = 0
    for b in range(B):
        c = overlaps.get_corners_of_cuboid(*[pt[b, :, i].contiguous() for i in range(7)]).cpu().numpy()
        m = _oracle_overlap3d(O, c)
        assert np.array_equal(exact_gpu[b].cpu().numpy(), m, equal_nan=True)             # exact-order kernel == oracle, bit for bit
        got = out[6][b].cpu().numpy()
        assert float(np.abs(got - m).max()) <= 2e-6
        # every `> thr` decision of the written matrix is the reference's; report how many pairs sat in the guard band
        assert np.array_equal(got > 0.4, m > 0.4)
        band = np.abs(m - np.float32(0.4)) <= 4e-6
        assert np.array_equal(got[band], m[band])
        ref = O.differentiable_nms(scores[b], m, grad_prob=w)
        prob = out[0][b].detach().cpu().numpy()
        nv, ni = int(out[4][b]), int(out[5][b])
        assert float(np.abs(prob - ref["prob"]).max()) <= 1e-4
        assert float(np.abs(st.grad[b].cpu().numpy() - ref["grad_scores"]).max()) <= 1e-4
        assert set(out[2][b, :nv].tolist()) == set(ref["valid"].tolist()) and nv == len(ref["valid"])
        assert set(out[3][b, :ni].tolist()) == set(ref["invalid"].tolist()) and ni == len(ref["invalid"])
        # the same from the RAW parameters with the oracle's OWN corners (libm sinf / cosf where the device has its own): the matrix
        # agrees to the corner rounding, and the index sets are compared too -- they can differ only through a pair whose overlap lies
        # within that rounding (~1e-6) of the threshold.  The flip count goes to gpurun_out/iou3d_raw_param_flips.jsonl; at most one
        # image of a case may differ.
        m2 = _oracle_overlap3d(O, O.corners_of_cuboid(par[b]))
        assert float(np.abs(got - m2).max()) <= 2e-5
        ref2 = O.differentiable_nms(scores[b], m2)
        pair_flips = int(((got > 0.4) != (m2 > 0.4)).sum())
        set_equal = set(out[2][b, :nv].tolist()) == set(ref2["valid"].tolist())
        _record("iou3d_raw_param_flips.jsonl", {"N": N, "clustered": bool(clustered), "image": b, "pairs_flipped_of_N2": pair_flips,
                                                 "valid_set_equal": bool(set_equal), "max_abs_dmatrix": float(np.abs(got - m2).max())})
        raw_diff += int(not set_equal)
        assert raw_diff <= 1, (N, clustered, b, pair_flips)
        if set_equal:
            assert float(np.abs(prob - ref2["prob"]).max()) <= 1e-4


@pytest.mark.parametrize("B,N,clustered", [(3, 256, True), (2, 258, False), (2, 1000, True), (2, 4096, True), (1, 5000, False), (1, 8192, True)])
def test_iou3d_symmetric_writer(G, O, B, N, clustered):
    """The symmetric 3D matrix writer (iou3d_sym_kernel: every unordered pair evaluated once, each 128 x 128 macro tile stored directly
    and mirrored through LDS) writes the SAME matrix as the all-pairs kernels of the one-call entry (iou3d_nms_fast_kernel /
    the bit-matrix kernels: one per-pair definition, iou3d_pair.h), bit for bit -- ragged last tiles, several images, thresholds whose guard
    band holds many pairs -- and the matrix is symmetric; against the oracle's exact operation order: within 2e-6, equal `> thr`
    decisions, equal entries inside the band."""
    from groomed_nms_amd import synthetic, overlaps
    par, scores = synthetic.batch_3d(900 + N, B, N, clustered=clustered, per=16)
    pt = torch.from_numpy(par).cuda()
    st = torch.from_numpy(scores).cuda()
    for thr in (0.4, 0.05, 0.75):
        m_sym = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True, nms_threshold=thr)        # gnms_nms_overlap3d_from_params
        m_all = G.differentiable_nms_with_iou3d_batched(st, pt, nms_threshold=thr)[6]                    # the one-call entry's writer
        assert torch.equal(m_sym, m_all), (N, thr, int((m_sym != m_all).sum()))
        assert torch.equal(m_sym, m_sym.transpose(1, 2))
    if N <= 4096:
        exact = overlaps.iou3d_batched(pt, from_params=True, nms_overlap=True)                           # exact-order kernel == oracle (tested above)
        got, ex = m_sym.cpu().numpy(), exact.cpu().numpy()
        assert float(np.abs(got - ex).max()) <= 2e-6 and np.array_equal(got > 0.75, ex > 0.75)
        band = np.abs(ex - np.float32(0.75)) <= 4e-6
        assert np.array_equal(got[band], ex[band])
    # a padded leading dimension and an odd one (the latter falls back to the all-pairs kernel): same entries
    import ctypes
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import ptr, check, stream_ptr
    lib = _lib.load()
    for ld in (N + 6, N + 3):
        buf = torch.full((B, N, ld), -7.0, device="cuda")
        check(lib.gnms_nms_overlap3d_from_params(ptr(pt), B, N, 0.75, ptr(buf), ld, stream_ptr(pt.device)), "overlap3d")
        assert torch.equal(buf[:, :, :N], m_sym) and bool((buf[:, :, N:] == -7.0).all()), ld


@pytest.mark.parametrize("B,N,kind", [(2, 4096, "clustered"), (2, 4096, "uniform"), (1, 16384, "clustered"), (1, 16384, "uniform")])
def test_iou2d_one_call_and_from_boxes_against_oracle_at_scale(G, O, B, N, kind):
    """The 2D one-call entry (gnms_forward_with_iou2d) and the matrix-free entry (gnms_forward_from_boxes) against the CPU oracle
    at BASELINE sizes: matrix, probabilities, valid list and score gradient bit for bit."""
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(57 + N, B, N, kind)
    bt = torch.from_numpy(boxes).cuda()
    w = np.linspace(-1, 2, N).astype(np.float32)
    wt = torch.from_numpy(w).cuda()
    s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
    s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
    o1 = G.differentiable_nms_with_iou2d_batched(s1, bt)
    o2 = G.differentiable_nms_from_boxes_batched(s2, bt)
    (o1[0] * wt).sum().backward()
    (o2[0] * wt).sum().backward()
    for b in range(B):
        m = O.iou2d(boxes[b], boxes[b])
        assert np.array_equal(o1[6][b].cpu().numpy(), m, equal_nan=True)
        ref = O.differentiable_nms(scores[b], m, grad_prob=w)
        for o, s in ((o1, s1), (o2, s2)):
            assert np.array_equal(o[0][b].detach().cpu().numpy(), ref["prob"])
            assert o[2][b, :int(o[4][b])].tolist() == list(ref["valid"])
            assert sorted(o[3][b, :int(o[5][b])].tolist()) == sorted(ref["invalid"].tolist())
            assert np.array_equal(s.grad[b].cpu().numpy(), ref["grad_scores"])


def test_separate_launch_tail_from_boxes_against_oracle(G, O):
    """gnms_forward_from_boxes, masked groups, ONE image of N = 4160 -- just past the fused tail's 4096, so K3..K6 run as launches of their
    own from the boxes (leaders, attribution, groups, finalize) -- against the CPU oracle: probabilities, valid list, counts and score
    gradient bit for bit, the invalid list as a set."""
    from groomed_nms_amd import synthetic
    N = 4160
    boxes, scores = synthetic.batch_2d(57 + N, 1, N, "clustered")
    w = np.linspace(-1, 2, N).astype(np.float32)
    s = torch.from_numpy(scores).cuda().requires_grad_(True)
    o = G.differentiable_nms_from_boxes_batched(s, torch.from_numpy(boxes).cuda())
    (o[0] * torch.from_numpy(w).cuda()).sum().backward()
    ref = O.differentiable_nms(scores[0], O.iou2d(boxes[0], boxes[0]), grad_prob=w)
    nv, ni = int(o[4][0]), int(o[5][0])
    assert np.array_equal(o[0][0].detach().cpu().numpy(), ref["prob"])
    assert nv == len(ref["valid"]) and ni == len(ref["invalid"])
    assert o[2][0, :nv].tolist() == list(ref["valid"])
    assert sorted(o[3][0, :ni].tolist()) == sorted(ref["invalid"].tolist())
    assert np.array_equal(s.grad[0].cpu().numpy(), ref["grad_scores"])


def test_separate_launch_tail_from_records_against_oracle(G, O):
    """gnms_forward_with_iou3d, masked groups, ONE image of N = 2112 at a threshold below the cull's 0.01 limit (0.005): the unculled
    bit-matrix kernel writes no symmetric rows, so past N = 2048 K3..K6 run as launches of their own from the records.  The written matrix
    against the oracle's exact operation order (within 2e-6, the same `> thr` decisions); and the layer against the oracle ON that matrix:
    probabilities, valid list, counts and score gradient bit for bit, the invalid list as a set (the layer decides every pair as the
    written entry does, and the masked linear mode has no transcendental)."""
    from groomed_nms_amd import synthetic, overlaps
    N, thr = 2112, 0.005
    par, scores = synthetic.batch_3d(31 + N, 1, N, clustered=True, per=64)
    pt = torch.from_numpy(par).cuda()
    w = np.linspace(-1, 2, N).astype(np.float32)
    s = torch.from_numpy(scores).cuda().requires_grad_(True)
    o = G.differentiable_nms_with_iou3d_batched(s, pt, nms_threshold=thr)
    (o[0] * torch.from_numpy(w).cuda()).sum().backward()
    got = o[6][0].cpu().numpy()
    c = overlaps.get_corners_of_cuboid(*[pt[0, :, i].contiguous() for i in range(7)]).cpu().numpy()
    exact = _oracle_overlap3d(O, c)
    assert float(np.abs(got - exact).max()) <= 2e-6 and np.array_equal(got > np.float32(thr), exact > np.float32(thr))
    ref = O.differentiable_nms(scores[0], got, grad_prob=w, nms_threshold=thr)
    nv, ni = int(o[4][0]), int(o[5][0])
    assert np.array_equal(o[0][0].detach().cpu().numpy(), ref["prob"])
    assert nv == len(ref["valid"]) and ni == len(ref["invalid"])
    assert o[2][0, :nv].tolist() == list(ref["valid"])
    assert sorted(o[3][0, :ni].tolist()) == sorted(ref["invalid"].tolist())
    assert np.array_equal(s.grad[0].cpu().numpy(), ref["grad_scores"])


def test_large_images_take_the_same_decisions(G):
    """B=8, N=8192 crosses every size switch at once: cooperative sorts (8 runs per image), 4 rank blocks per bit-matrix wave,
    separate K3..K6 launches.  One-call entry, matrix-free entry and matrix-in entry must agree bit for bit."""
    from groomed_nms_amd import synthetic, overlaps
    _large_image_case(G, 8, 8192, [8192, 8191, 5000, 4097, 8000, 64, 1, 7777])
    _large_image_case(G, 2, 16384, [16384, 9001])             # the largest image the library takes: 16 sort runs, 256 rank blocks


def _large_image_case(G, B, N, count_list):
    from groomed_nms_amd import synthetic, overlaps
    boxes, scores = synthetic.batch_2d(21, B, N, "clustered", per=48)
    bt = torch.from_numpy(boxes).cuda()
    counts = torch.tensor(count_list, dtype=torch.int32).cuda()
    w = torch.rand((B, N), device="cuda")
    outs, grads = [], []
    for fn in (lambda s: G.differentiable_nms_with_iou2d_batched(s, bt, counts=counts),
               lambda s: G.differentiable_nms_from_boxes_batched(s, bt, counts=counts),
               lambda s: G.differentiable_nms_batched(s, overlaps.iou_batched(bt), counts=counts)):
        s = torch.from_numpy(scores).cuda().requires_grad_(True)
        out = fn(s)
        (out[0] * w).sum().backward()
        outs.append([o.detach().clone() for o in out[:6]])
        grads.append(s.grad.clone())
        del out
    for k in (1, 2):
        for a, b in zip(outs[0], outs[k]):
            assert torch.equal(a, b)
        assert torch.equal(grads[0], grads[k])
    assert int(outs[0][4].sum()) > 0


def test_batches_past_two_to_the_32_matrix_elements(G):
    """32 images x 16384 boxes = 2^33 matrix elements (32 GiB), 2D and 3D: every offset into the matrix is 64-bit.  Images of the
    big batch must come out exactly as when they are run alone (outputs, score gradient, matrix)."""
    from groomed_nms_amd import synthetic
    B, N = 32, 16384
    for dim in (2, 3):
        if dim == 2:
            boxes, scores = synthetic.batch_2d(5, B, N, "clustered", per=48)
            fn = G.differentiable_nms_with_iou2d_batched
        else:
            boxes, scores = synthetic.batch_3d(5, B, N, True)
            fn = G.differentiable_nms_with_iou3d_batched
        bt = torch.from_numpy(boxes).cuda(); st = torch.from_numpy(scores).cuda().requires_grad_(True)
        w = torch.rand((B, N), device="cuda")
        out = fn(st, bt)
        (out[0] * w).sum().backward()
        assert out[6].shape == (B, N, N)
        for img in (B - 1, B // 2):
            s1 = torch.from_numpy(scores[img:img + 1]).cuda().requires_grad_(True)
            o1 = fn(s1, bt[img:img + 1])
            (o1[0] * w[img:img + 1]).sum().backward()
            for a, b in zip(out[:6], o1[:6]):
                assert torch.equal(a[img:img + 1], b), (dim, img)
            assert torch.equal(st.grad[img:img + 1], s1.grad)
            assert torch.equal(out[6][img], o1[6][0])
        assert int(out[4].sum()) > 0
        del out, o1
        torch.cuda.empty_cache()


def test_host_threads_share_the_side_stream(G):
    """Three host threads, each on its own torch stream, call the large-image one-call entries at once: the library's side
    stream and its fork/join events are shared per device, every result must still equal the single-threaded one."""
    import threading
    from groomed_nms_amd import synthetic

    def make(seed, dim, B, N):
        if dim == 2:
            b, s = synthetic.batch_2d(seed, B, N, "clustered", per=48)
            return G.differentiable_nms_with_iou2d_batched, torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
        b, s = synthetic.batch_3d(seed, B, N, True)
        return G.differentiable_nms_with_iou3d_batched, torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()

    cases = [make(1, 2, 2, 8192), make(2, 3, 2, 8192), make(3, 2, 1, 16384)]
    refs = []
    for fn, b, s in cases:
        sg = s.clone().requires_grad_(True)
        out = fn(sg, b)
        out[0].sum().backward()
        refs.append(([o.clone() for o in out[:7]], sg.grad.clone()))
    torch.cuda.synchronize()
    errors = []

    def worker(tid):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for it in range(6):
                k = (tid + it) % len(cases)
                fn, b, s = cases[k]
                sg = s.clone().requires_grad_(True)
                out = fn(sg, b)
                out[0].sum().backward()
                st.synchronize()
                if not all(torch.equal(a, r) for a, r in zip(out[:7], refs[k][0])) or not torch.equal(sg.grad, refs[k][1]):
                    errors.append((tid, it, k))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors[:5]


@pytest.mark.gpu
def test_one_launch_under_threads_and_streams(G):
    """Round 6: six host threads, each on its own torch stream, call both small-image entries at once -- the matrix-in layer (one_launch_kernel)
    and the one-call entry (one_launch_boxes_kernel: its matrix writers claim their tiles from a per-stream slot of the library's claim ring) --
    on images of different sizes, each call with a workspace of its own: flags, call counters and claim slots of concurrent launches must not
    meet.  Every result equals the single-threaded one bit for bit."""
    import threading
    from groomed_nms_amd import synthetic, overlaps
    cases = []
    for seed, B, N in ((1, 1, 500), (2, 2, 300), (3, 8, 256), (4, 1, 1024), (5, 3, 65), (6, 2, 512)):
        b, s = synthetic.batch_2d(seed, B, N, "clustered", per=20)
        cases.append((torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()))
    refs = []
    for b, s in cases:
        sg = s.clone().requires_grad_(True)
        one = G.differentiable_nms_with_iou2d_batched(sg, b)
        one[0].sum().backward()
        g1 = sg.grad.clone()
        sg2 = s.clone().requires_grad_(True)
        two = G.differentiable_nms_batched(sg2, overlaps.iou_batched(b))
        two[0].sum().backward()
        refs.append(([o.clone() for o in one[:7]], g1, [o.clone() for o in two[:6]], sg2.grad.clone()))
    torch.cuda.synchronize()
    errors = []

    def worker(tid):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for it in range(40):
                k = (tid + it) % len(cases)
                b, s = cases[k]
                sg = s.clone().requires_grad_(True)
                if (tid + it) % 2:
                    out = G.differentiable_nms_with_iou2d_batched(sg, b)
                    want, wg = refs[k][0], refs[k][1]
                else:
                    out = G.differentiable_nms_batched(sg, overlaps.iou_batched(b))
                    want, wg = refs[k][2], refs[k][3]
                out[0].sum().backward()
                st.synchronize()
                if not all(torch.equal(a, r) for a, r in zip(out, want)) or not torch.equal(sg.grad, wg):
                    errors.append((tid, it, k))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors[:5]


def test_api_edges(G):
    """What callers actually hand over: strided views, float64, a padded leading dimension, a matrix that requires grad, NumPy
    float64 in / CPU tensors out (lib/rpn_util.py:1319-1320), empty inputs, an unknown pruning method, impossible shapes."""
    from groomed_nms_amd import synthetic, overlaps, _lib
    boxes, scores = synthetic.batch_2d(3, 2, 300, "clustered", per=20)
    bt = torch.from_numpy(boxes).cuda(); st = torch.from_numpy(scores).cuda()
    ref = G.differentiable_nms_with_iou2d_batched(st, bt)

    def same(out):
        for a, b in zip(out[:6], ref[:6]):
            assert torch.equal(a, b)
    big = torch.zeros((2, 300, 6), device="cuda"); big[..., 1:5] = bt
    same(G.differentiable_nms_with_iou2d_batched(st, big[..., 1:5]))                     # strided boxes
    sbig = torch.zeros((2, 600), device="cuda"); sbig[:, ::2] = st
    same(G.differentiable_nms_with_iou2d_batched(sbig[:, ::2], bt))                      # strided scores
    same(G.differentiable_nms_with_iou2d_batched(st.double(), bt.double()))              # float64 -> computed in fp32
    iou = overlaps.iou_batched(bt)
    pad = torch.zeros((2, 300, 304), device="cuda"); pad[..., :300] = iou
    same(G.differentiable_nms_batched(st, pad[..., :300]))                               # leading dimension 304
    iou_g = iou.clone().requires_grad_(True); s_g = st.clone().requires_grad_(True)
    out = G.differentiable_nms_batched(s_g, iou_g)
    (out[0] * torch.rand_like(out[0])).sum().backward()
    assert iou_g.grad.shape == iou.shape and float(iou_g.grad.abs().sum()) > 0           # sparse dL/diou
    v, iv, p = G.differentiable_nms(scores[0].astype(np.float64), iou[0].cpu().numpy())
    assert not p.is_cuda and p.shape == (300,) and v.dtype == torch.int64 and len(v) + len(iv) == 300
    v, iv, p = G.differentiable_nms(torch.zeros(0, device="cuda"), torch.zeros((0, 0), device="cuda"))
    assert v.numel() == 0 and iv.numel() == 0 and p.numel() == 0
    out = G.differentiable_nms_with_iou2d_batched(torch.zeros((0, 5), device="cuda"), torch.zeros((0, 5, 4), device="cuda"))
    assert out[0].shape == (0, 5)
    with pytest.raises(NotImplementedError, match="Pruning method not implemented!"):       # lib/groomed_nms.py:177-178
        G.differentiable_nms(torch.rand(5, device="cuda"), torch.rand((5, 5), device="cuda"), pruning_method="bogus")
    with pytest.raises(_lib.GnmsError):
        G.differentiable_nms_batched(torch.rand((1, 20000), device="cuda"), torch.rand((1, 4, 4), device="cuda"))


def test_make_graphed_callables(G):
    """The Python layer (autograd.Function over the C ABI) survives torch.cuda.make_graphed_callables: forward and backward are
    captured into HIP graphs once and replayed on new scores with the same results and gradients as eager calls."""
    from groomed_nms_amd import synthetic
    B, N = 4, 500
    boxes_np, scores_np = synthetic.batch_2d(5, B, N, "clustered", per=25)
    boxes = torch.from_numpy(boxes_np).cuda()

    class Layer(torch.nn.Module):
        def forward(self, scores, bx):
            return G.differentiable_nms_with_iou2d_batched(scores, bx)[0]
    layer = Layer()
    graphed = torch.cuda.make_graphed_callables(layer, (torch.from_numpy(scores_np).cuda().requires_grad_(True), boxes))
    w = torch.rand((B, N), device="cuda")
    for trial in range(3):
        _, sc = synthetic.batch_2d(50 + trial, B, N, "clustered", per=25)
        s1 = torch.from_numpy(sc).cuda().requires_grad_(True)
        s2 = torch.from_numpy(sc).cuda().requires_grad_(True)
        p1 = graphed(s1, boxes)
        (p1 * w).sum().backward()
        p2 = layer(s2, boxes)
        (p2 * w).sum().backward()
        assert torch.equal(p1, p2) and torch.equal(s1.grad, s2.grad) and float(p1.detach().sum()) > 0


def test_probabilities_only_mode(G):
    """index_lists=False (valid / invalid NULL in the C ABI): same probabilities, counts and gradients, no lists."""
    from groomed_nms_amd import synthetic, overlaps
    for B, N in ((3, 700), (2, 4096)):
        boxes, scores = synthetic.batch_2d(31, B, N, "clustered", per=32)
        bt = torch.from_numpy(boxes).cuda()
        w = torch.rand((B, N), device="cuda")
        for fn in (lambda s, **k: G.differentiable_nms_with_iou2d_batched(s, bt, **k),
                   lambda s, **k: G.differentiable_nms_from_boxes_batched(s, bt, **k),
                   lambda s, **k: G.differentiable_nms_batched(s, overlaps.iou_batched(bt), **k)):
            s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
            s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
            full = fn(s1)
            lean = fn(s2, index_lists=False)
            assert lean[2] is None and lean[3] is None
            assert torch.equal(full[0], lean[0]) and torch.equal(full[1], lean[1])
            assert torch.equal(full[4], lean[4]) and torch.equal(full[5], lean[5])
            (full[0] * w).sum().backward()
            (lean[0] * w).sum().backward()
            assert torch.equal(s1.grad, s2.grad)


# ------------------------------------------------------------------------------------------------
# round 2: advisor findings, distributed plumbing on the box
# ------------------------------------------------------------------------------------------------
def test_pruning_function_is_differentiable(G, O):
    """pruning_function composes in an autograd graph like the reference's plain torch ops (lib/groomed_nms.py:167-189)."""
    x = torch.rand((37, 41), device="cuda", dtype=torch.float32, requires_grad=True)
    for method, temp in (("sigmoidal", 0.1), ("soft_nms", 0.5), ("linear", 0.01)):
        x.grad = None
        y = G.pruning_function(x, 0.4, temp, method)
        assert y.requires_grad
        g = torch.rand_like(y)
        (y * g).sum().backward()
        xd = x.detach().double()
        if method == "sigmoidal":
            sg = torch.sigmoid((xd - 0.4) / temp)
            ref = sg * (1 - sg) / temp
        elif method == "soft_nms":
            ref = torch.exp(-xd * xd / temp) * 2 * xd / temp
        else:
            ref = torch.ones_like(xd)
        np.testing.assert_allclose(x.grad.cpu().numpy(), (ref * g.double()).float().cpu().numpy(), atol=2e-6, rtol=2e-6)
    xc = torch.rand(16, requires_grad=True)                                    # CPU tensor in -> CPU tensor out, gradient on the CPU leaf
    G.pruning_function(xc, 0.4, 0.1, "sigmoidal").sum().backward()
    assert xc.grad is not None and xc.grad.device.type == "cpu" and float(xc.grad.abs().sum()) > 0


def test_soft_sort_rectangular_matrix(G, O):
    """soft_sort accepts any [N, K] matrix like the reference's matmul (:163); wrong row counts raise instead of reading out of bounds."""
    rng = np.random.default_rng(4)
    n, k = 70, 33
    s = np.sort(rng.uniform(size=n).astype(np.float32))[::-1].copy()
    m = rng.uniform(size=(n, k)).astype(np.float32)
    ss, C, sm = G.soft_sort(torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda(), 0.05)
    _, oC, _ = O.soft_sort(s, None, 0.05)
    np.testing.assert_allclose(C.cpu().numpy(), oC, atol=2e-5)
    np.testing.assert_allclose(sm.cpu().numpy(), oC.astype(np.float64) @ m.astype(np.float64), atol=2e-5)
    assert sm.shape == (n, k)
    with pytest.raises(ValueError):
        G.soft_sort(torch.from_numpy(s).cuda(), torch.from_numpy(m[:-1]).cuda(), 0.05)


def test_overwritten_matrix_buffer_is_caught(G):
    """The ungrouped backward reads the overlap matrix: a caller that overwrites the iou_out buffer between forward and backward gets
    autograd's version-counter error, not silently wrong gradients.  The masked default never reads it, and the grouped unmasked
    backward solves its groups from the boxes (round 4b): both are unaffected, gradients identical to a run that left the buffer alone."""
    from groomed_nms_amd import synthetic
    boxes, scores = synthetic.batch_2d(3, 2, 300, "clustered", per=20)
    bt = torch.from_numpy(boxes).cuda()
    buf = torch.empty((2, 300, 300), device="cuda")
    s = torch.from_numpy(scores).cuda().requires_grad_(True)
    out = G.differentiable_nms_with_iou2d_batched(s, bt, iou_out=buf, group_boxes=False)
    buf.zero_()
    with pytest.raises(RuntimeError):
        out[0].sum().backward()
    for kw in (dict(), dict(mask_group_boxes=False)):
        s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
        s3 = torch.from_numpy(scores).cuda().requires_grad_(True)
        out = G.differentiable_nms_with_iou2d_batched(s2, bt, iou_out=buf, **kw)
        ref = G.differentiable_nms_with_iou2d_batched(s3, bt, **kw)
        buf.zero_()
        out[0].sum().backward()
        ref[0].sum().backward()
        assert torch.isfinite(s2.grad).all() and torch.equal(out[0], ref[0]) and torch.equal(s2.grad, s3.grad), kw


def test_ungrouped_block_solves_against_oracle(G, O):
    """group_boxes=False (lib/groomed_nms.py:110-111: inverse(I + P) @ scores): the two triangular solves on blocks of 128 positions
    with the diagonal tiles' inverses (csrc/nms_solve_kernels.h), ragged batches whose counts sit on, beside and far from the block
    edges, against the oracle's inverse in double.  Tolerances: TOL on the probabilities (north_star), 5e-4 / 1e-3 on the gradients
    as in test_random_vs_oracle."""
    from groomed_nms_amd import synthetic, overlaps
    rng = np.random.default_rng(2024)
    for N, counts, kind in ((300, [300, 129, 128, 127, 1, 0, 257, 256], "clustered"), (1000, [1000, 897, 896, 641], "uniform"),
                            (2048, [2048, 1500], "clustered")):
        B = len(counts)
        boxes = np.stack([(synthetic.clustered_boxes_2d(rng, N, 24) if kind == "clustered" else synthetic.uniform_boxes_2d(rng, N))
                          for _ in range(B)])
        scores = np.stack([synthetic.tie_free_scores(rng, N) for _ in range(B)])
        w = rng.uniform(-1, 2, size=(B, N)).astype(np.float32)
        ct = torch.from_numpy(np.array(counts, np.int32)).cuda()
        for mode in ("un_lin", "un_sig"):
            st = torch.from_numpy(scores).cuda().requires_grad_(True)
            iou = overlaps.iou_batched(torch.from_numpy(boxes).cuda()).requires_grad_(N <= 300)
            prob, order, valid, invalid, nv, ni = G.differentiable_nms_batched(st, iou, counts=ct, **MODES[mode])
            (prob * torch.from_numpy(w).cuda()).sum().backward()
            for b in range(B):
                n = counts[b]
                tag = f"N={N} n={n} {mode}"
                assert torch.all(st.grad[b, n:] == 0) and torch.all(prob[b, n:] == 0), tag
                if n == 0:
                    assert int(nv[b]) == 0 and int(ni[b]) == 0, tag
                    continue
                m = O.iou2d(boxes[b, :n], boxes[b, :n])
                ref = O.differentiable_nms(scores[b, :n], m, grad_prob=w[b, :n], want_grad_iou=(N <= 300), **MODES[mode])
                np.testing.assert_allclose(prob[b, :n].detach().cpu().numpy(), ref["prob"], atol=TOL, err_msg=tag)
                np.testing.assert_allclose(st.grad[b, :n].cpu().numpy(), ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=tag)
                check_index_lists(valid[b, :int(nv[b])].cpu().numpy(), invalid[b, :int(ni[b])].cpu().numpy(), ref["valid"], ref["invalid"])
                if N <= 300:
                    np.testing.assert_allclose(iou.grad[b, :n, :n].cpu().numpy(), ref["grad_iou"], atol=5e-4, rtol=1e-3, err_msg=tag)


def test_ungrouped_matrix_from_boxes_plain_and_other_boxes(G):
    """ungrouped_permute_boxes_kernel takes the matrix writers' packed row body when every box of a wave's work "divides plainly"
    (csrc/iou_tile.h) and pair_iou's IEEE division otherwise; either way the pruned triangular matrix must equal, bit for bit, what the
    matrix-in entry permutes out of gnms_iou2d's matrix (lib/core.py:480-508).  Pixel boxes (plain), the same boxes scaled beyond 2^20
    (not plain), a batch with one box moved to a negative-zero corner and one zero-area box (NaN self-overlap is never read: j < i)."""
    from groomed_nms_amd import synthetic, overlaps
    rng = np.random.default_rng(4242)
    for N, scale, poke in ((333, 1.0, False), (333, 4.0e6, False), (260, 1.0, True), (700, 3.0e-5, False)):
        boxes, scores = synthetic.batch_2d(int(rng.integers(1 << 30)), 2, N, "clustered", per=6)
        boxes = (boxes * np.float32(scale)).astype(np.float32)
        if poke:
            boxes[0, 5, 0] = -0.0
            boxes[1, 7] = boxes[1, 7, [0, 1, 0, 1]]                       # zero area
        bt = torch.from_numpy(boxes).cuda()
        w = torch.from_numpy(rng.uniform(-1, 2, (2, N)).astype(np.float32)).cuda()
        s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
        s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
        one = G.differentiable_nms_with_iou2d_batched(s1, bt, group_boxes=False)
        two = G.differentiable_nms_batched(s2, overlaps.iou_batched(bt), group_boxes=False)
        (one[0] * w).sum().backward()
        (two[0] * w).sum().backward()
        tag = (N, scale, poke)
        assert torch.equal(one[0], two[0]) or torch.allclose(one[0], two[0], atol=0, rtol=0, equal_nan=True), tag
        assert torch.equal(s1.grad, s2.grad) or torch.allclose(s1.grad, s2.grad, atol=0, rtol=0, equal_nan=True), tag


def test_ungrouped_mode_with_a_tight_workspace(G, O):
    """Ungrouped mode at sizes that are not multiples of 64, through the C ABI with a workspace of EXACTLY gnms_workspace_bytes that
    ends at the end of its allocation (the diagonal-tile loads of the last row block stay inside the scratch pitch)."""
    import ctypes
    from groomed_nms_amd import synthetic, _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, check
    lib = _lib.load()
    rng = np.random.default_rng(8)
    for n in (65, 100, 130, 191):
        b = synthetic.clustered_boxes_2d(rng, n, 8)
        s = synthetic.tie_free_scores(rng, n)
        m = O.iou2d(b, b)
        w = rng.uniform(-1, 2, size=n).astype(np.float32)
        P = GnmsParams()
        lib.gnms_default_params(ctypes.byref(P))
        P.group_boxes = 0
        nbytes = lib.gnms_workspace_bytes(1, n, ctypes.byref(P))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        st, mt, wt = torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
        prob = torch.empty(n, device="cuda"); gs = torch.empty(n, device="cuda")
        check(lib.gnms_forward(ptr(st), ptr(mt), 1, n, n, None, ctypes.byref(P), ptr(prob), None, None, None, None, None, ptr(ws), nbytes, None), "fwd")
        check(lib.gnms_backward(ptr(wt), ptr(st), ptr(mt), 1, n, n, None, ctypes.byref(P), ptr(gs), None, ptr(ws), nbytes, None), "bwd")
        torch.cuda.synchronize()
        ref = O.differentiable_nms(s, m, grad_prob=w, group_boxes=False)
        np.testing.assert_allclose(prob.cpu().numpy(), ref["prob"], atol=TOL)
        np.testing.assert_allclose(gs.cpu().numpy(), ref["grad_scores"], atol=5e-4, rtol=1e-3)


def _run_py(code, env_extra, timeout=600, argv=()):
    import os, subprocess, sys
    env = dict(os.environ)
    env.update(env_extra)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, "-c", code] + list(argv), cwd=root, env=env, capture_output=True, text=True, timeout=timeout)


def test_rccl_single_rank_plumbing():
    """GNMS_FORCE_DIST=1: init RCCL (backend nccl) with one rank on this GPU, run the per-step heartbeat all-reduce, the MAX/SUM
    reductions of the timing contract and a timed region around the HIP layer -- the collective plumbing bench.py uses at N > 1."""
    from test_distributed_gloo import _free_port
    code = """
import torch, numpy as np
from groomed_nms_amd import dist as gdist, synthetic
import groomed_nms_amd as G
world, rank, lr = gdist.init(backend="nccl")
import torch.distributed as dist
assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
torch.cuda.set_device(lr)
b, s = synthetic.batch_2d(1, 2, 512, "clustered", per=16)
bt, st = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda().requires_grad_(True)
hb = gdist.StepHeartbeat()
def step():
    p = G.differentiable_nms_with_iou2d_batched(st, bt)[0]
    st.grad = None
    p.sum().backward()
dt = gdist.timed_steps(step, 5, 2, torch.cuda.synchronize, hb)
assert dt > 0 and hb.steps == 7
assert gdist.max_over_ranks(3.5) == 3.5 and gdist.sum_over_ranks(2.0) == 2.0
gdist.barrier()
dist.destroy_process_group()
print("RCCL_OK", dt)
"""
    r = _run_py(code, {"GNMS_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(_free_port()), "RANK": "0", "WORLD_SIZE": "1",
                       "LOCAL_RANK": "0", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _hip_shard_worker(rank, world, port, total, n, out_dir):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from groomed_nms_amd import dist as gdist, synthetic
    import groomed_nms_amd as G
    gdist.init(backend="gloo")                      # two ranks share the box's one GPU: gloo carries the collectives, HIP the layer
    torch.cuda.set_device(0)
    boxes, scores = synthetic.batch_2d(42, total, n, "clustered", per=16)
    lo, hi = gdist.shard_range(total, rank, world)
    bt = torch.from_numpy(boxes[lo:hi]).cuda()
    st = torch.from_numpy(scores[lo:hi]).cuda().requires_grad_(True)
    hb = gdist.StepHeartbeat(torch.device("cpu"))
    keep = {}

    def step():
        out = G.differentiable_nms_with_iou2d_batched(st, bt)
        st.grad = None
        out[0].sum().backward()
        keep["prob"], keep["grad"] = out[0].detach(), st.grad

    gdist.timed_steps(step, 3, 1, torch.cuda.synchronize, hb)
    assert gdist.sum_over_ranks(float(hi - lo), torch.device("cpu")) == float(total)
    np.save(os.path.join(out_dir, "prob%d.npy" % rank), keep["prob"].cpu().numpy())
    np.save(os.path.join(out_dir, "grad%d.npy" % rank), keep["grad"].cpu().numpy())
    gdist.barrier()
    dist.destroy_process_group()


def test_two_ranks_shard_the_hip_layer(G, O, tmp_path):
    """world_size 2 (gloo collectives, both ranks on this box's GPU): every rank runs the HIP layer on ITS contiguous slice of the
    images; the concatenated results equal the oracle's on the whole batch, bit for bit; the heartbeat saw every step of every rank."""
    import os
    import torch.multiprocessing as mp
    from groomed_nms_amd import synthetic
    from test_distributed_gloo import _free_port
    world, total, n = 2, 5, 640
    mp.spawn(_hip_shard_worker, args=(world, _free_port(), total, n, str(tmp_path)), nprocs=world, join=True)
    prob = np.concatenate([np.load(os.path.join(tmp_path, "prob%d.npy" % r)) for r in range(world)])
    grad = np.concatenate([np.load(os.path.join(tmp_path, "grad%d.npy" % r)) for r in range(world)])
    boxes, scores = synthetic.batch_2d(42, total, n, "clustered", per=16)
    for b in range(total):
        ref = O.differentiable_nms(scores[b], O.iou2d(boxes[b], boxes[b]), grad_prob=np.ones(n, np.float32))
        assert np.array_equal(prob[b], ref["prob"]) and np.array_equal(grad[b], ref["grad_scores"]), b


def test_bench_refuses_more_gpus_than_the_node_has():
    """`python bench.py --gpus K` starts K ranks itself; with fewer visible GPUs it must fail loudly, never time fewer and report K."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    have = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(have + 1), "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], env=env2,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_float64_numpy_call_site(G, golden_f64site):
    """The reference's inference call site with its float64 NumPy arguments (lib/rpn_util.py:1292-1320), N = 500, 200 2D + 60 3D
    seeded cases against vectors generated by the imported reference (tests/golden/make_golden.py::make_f64_call_site):
      2D  overlaps.iou(float64 ndarray) -> float64 matrix, bit-identical to the reference's (SHA-256) on every case ->
          differentiable_nms(ndarray, ndarray): the reference's keep sets and probabilities, every case;
      3D  overlaps.get_corners_of_cuboid(float32 ndarrays) -> float64 corners -> .float() -> iou3d_approximate -> 0.5 (1 + giou) ->
          differentiable_nms: keep sets equal wherever the fp32-rounded corners are the reference's (np.cos on float32 is a SIMD kernel
          of the reference's host; the device's cosf may differ in the last bit), and at most a documented handful of cases elsewhere.
    Also counts what the fp32-on-GPU evaluation of the same float64 proposals would have changed (the path before this round) and
    leaves the figures in gpurun_out/f64site_flips.json."""
    import hashlib, json, os
    from conftest import f64site_aboxes
    from groomed_nms_amd import overlaps
    g = golden_f64site
    off = g["d2/valid_off"]
    ncase = g["d2/boxes32"].shape[0]
    flips32, entries32 = 0, 0
    for c in range(ncase):
        ab = f64site_aboxes(g, c)
        m = overlaps.iou(ab[:, 0:4], ab[:, 0:4], mode='combinations')                   # lib/rpn_util.py:1295
        assert isinstance(m, np.ndarray) and m.dtype == np.float64
        assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).digest() == g["d2/iou_sha256"][c].tobytes(), c
        keep, _, scores_new = G.differentiable_nms(scores_unsorted=ab[:, 4], iou_unsorted=m, nms_threshold=0.4)     # :1319
        assert keep.device.type == "cpu"
        want = g["d2/valid"][off[c]:off[c + 1]]
        assert sorted(keep.numpy().tolist()) == sorted(want.tolist()), c
        assert np.array_equal(scores_new.numpy(), g["d2/prob"][c]), c
        # the fp32-on-GPU evaluation of the same proposals (what overlaps.iou did with float64 input before)
        m32 = overlaps.iou(ab[:, 0:4].astype(np.float32), ab[:, 0:4].astype(np.float32), mode='combinations')
        entries32 += int((m32 != m.astype(np.float32)).sum())
        k32 = G.differentiable_nms(ab[:, 4], m32, nms_threshold=0.4)[0]
        flips32 += int(sorted(k32.numpy().tolist()) != sorted(want.tolist()))
    off = g["d3/valid_off"]
    n3 = g["d3/params32"].shape[0]
    same_corners, set_diff, set_diff_same_corners, max_dprob = 0, 0, 0, 0.0
    for c in range(n3):
        raw = g["d3/params32"][c]
        corners = overlaps.get_corners_of_cuboid(raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4], raw[:, 5], raw[:, 6])   # :1303-1309
        assert isinstance(corners, np.ndarray) and corners.dtype == np.float64 and corners.shape == (500, 3, 8)
        c32 = torch.from_numpy(corners).float().cuda()                                   # :1310
        if g.has(f"d3/corners32_{c}"):
            assert np.abs(c32.cpu().numpy() - g[f"d3/corners32_{c}"]).max() <= 1e-5
        same = hashlib.sha256(np.ascontiguousarray(c32.cpu().numpy()).tobytes()).digest() == g["d3/corners32_sha256"][c].tobytes()
        _, i3 = overlaps.iou3d_approximate(c32, c32, mode="combinations", method="generalized")                  # :1311
        ious = (0.5 * (1 + i3)).cpu().numpy()                                            # :1312-1313
        keep, _, scores_new = G.differentiable_nms(scores_unsorted=g["d3/scores32"][c].astype(np.float64), iou_unsorted=ious, nms_threshold=0.4)
        eq = sorted(keep.numpy().tolist()) == sorted(g["d3/valid"][off[c]:off[c + 1]].tolist())
        same_corners += int(same)
        set_diff += int(not eq)
        set_diff_same_corners += int(same and not eq)
        if eq:
            max_dprob = max(max_dprob, float(np.abs(scores_new.numpy() - g["d3/prob"][c]).max()))
    rec = {"d2_cases": ncase, "d2_float64_path_matrix_bit_identical": ncase, "d2_float64_path_keep_set_differences": 0,
           "d2_fp32_path_matrix_entries_off_by_an_ulp": entries32, "d2_fp32_path_keep_set_differences": flips32,
           "d3_cases": n3, "d3_cases_with_the_reference_s_fp32_corners": same_corners, "d3_keep_set_differences": set_diff,
           "d3_max_abs_dprob_where_sets_agree": max_dprob}
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "f64site_flips.json"), "w") as f:
        json.dump(rec, f)
    print("f64site:", rec)
    assert set_diff_same_corners == 0 and set_diff <= 3 and max_dprob <= 1e-4, rec


def test_ctypes_binding_still_serves_the_layer():
    """The layer's default host path is the C++ binding (gnms_torch); the ctypes + torch.autograd.Function path over the same C ABI is
    the fallback (GNMS_BINDING=ctypes).  Both must give the oracle's results: a child process runs the four batched entries through
    ctypes -- forward, index lists, backward -- and compares them bit for bit with what this process gets through the binding.
    The B = 2, N = 200 cases are about what each binding keeps for the backward and which backward entry it calls (both ask
    gnms_backward_reads): from the boxes, from the kept matrix (2D ungrouped, 3D unmasked), and a box view at data_ptr() % 16 == 4."""
    import os, subprocess, sys, tempfile
    from groomed_nms_amd import synthetic, groomed_nms as GN, overlaps
    assert GN._binding(), "the C++ binding is not in use in this process"
    code = """
import sys, numpy as np, torch
from groomed_nms_amd import synthetic, groomed_nms as GN, overlaps
assert not GN._binding()
b, s = synthetic.batch_2d(77, 3, 700, "clustered", per=20)
p3, s3 = synthetic.batch_3d(78, 2, 600, clustered=True, per=12)
out = {}
def run(tag, fn, sc, *a, **kw):
    st = torch.from_numpy(sc).cuda().requires_grad_(True)
    o = fn(st, *a, **kw)
    (o[0] * torch.linspace(-1, 2, sc.shape[1], device="cuda")).sum().backward()
    out[tag + "/prob"] = o[0].detach().cpu().numpy(); out[tag + "/valid"] = o[2].cpu().numpy(); out[tag + "/nv"] = o[4].cpu().numpy()
    out[tag + "/grad"] = st.grad.cpu().numpy()
bt = torch.from_numpy(b).cuda()
run("with2d", GN.differentiable_nms_with_iou2d_batched, s, bt)
run("boxes", GN.differentiable_nms_from_boxes_batched, s, bt)
run("matrix", GN.differentiable_nms_batched, s, overlaps.iou_batched(bt))
run("unmasked", GN.differentiable_nms_batched, s, overlaps.iou_batched(bt), mask_group_boxes=False)
run("with3d", GN.differentiable_nms_with_iou3d_batched, s3, torch.from_numpy(p3).cuda())
# what each binding keeps for the backward, and the backward entry it then calls (gnms_backward_reads)
b2, s2 = synthetic.batch_2d(79, 2, 200, "clustered", per=20)
p2, s4 = synthetic.batch_3d(80, 2, 200, clustered=True, per=20)
cnt = torch.tensor([200, 137], dtype=torch.int32).cuda()
bt2 = torch.from_numpy(b2).cuda()
off = torch.empty((2 * 200 * 4 + 4,), device="cuda")[1:1601].view(2, 200, 4).copy_(bt2)      # a view one float into a larger buffer
assert off.data_ptr() % 16 == 4 and off.is_contiguous()
run("with2d_boxes_bwd", GN.differentiable_nms_with_iou2d_batched, s2, bt2, counts=cnt, mask_group_boxes=False)
run("with2d_matrix_bwd", GN.differentiable_nms_with_iou2d_batched, s2, bt2, counts=cnt, group_boxes=False)
try:
    run("with2d_unaligned", GN.differentiable_nms_with_iou2d_batched, s2, off, counts=cnt, mask_group_boxes=False)
    out["with2d_unaligned/error"] = np.array("")
except GN._lib.GnmsError as e:
    out["with2d_unaligned/error"] = np.array(str(e))
run("with3d_unmasked", GN.differentiable_nms_with_iou3d_batched, s4, torch.from_numpy(p2).cuda(), counts=cnt, mask_group_boxes=False)
np.savez(sys.argv[1], **out)
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ctypes.npz")
        r = _run_py(code, {"GNMS_BINDING": "ctypes"}, argv=[path])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        ref = np.load(path)
        b, s = synthetic.batch_2d(77, 3, 700, "clustered", per=20)
        p3, s3 = synthetic.batch_3d(78, 2, 600, clustered=True, per=12)
        bt = torch.from_numpy(b).cuda()

        def run(tag, fn, sc, *a, **kw):
            st = torch.from_numpy(sc).cuda().requires_grad_(True)
            o = fn(st, *a, **kw)
            (o[0] * torch.linspace(-1, 2, sc.shape[1], device="cuda")).sum().backward()
            assert np.array_equal(o[0].detach().cpu().numpy(), ref[tag + "/prob"], equal_nan=True), tag
            assert np.array_equal(o[2].cpu().numpy(), ref[tag + "/valid"]) and np.array_equal(o[4].cpu().numpy(), ref[tag + "/nv"]), tag
            assert np.array_equal(st.grad.cpu().numpy(), ref[tag + "/grad"]), tag
        run("with2d", GN.differentiable_nms_with_iou2d_batched, s, bt)
        run("boxes", GN.differentiable_nms_from_boxes_batched, s, bt)
        run("matrix", GN.differentiable_nms_batched, s, overlaps.iou_batched(bt))
        run("unmasked", GN.differentiable_nms_batched, s, overlaps.iou_batched(bt), mask_group_boxes=False)
        run("with3d", GN.differentiable_nms_with_iou3d_batched, s3, torch.from_numpy(p3).cuda())
        b2, s2 = synthetic.batch_2d(79, 2, 200, "clustered", per=20)
        p2, s4 = synthetic.batch_3d(80, 2, 200, clustered=True, per=20)
        cnt = torch.tensor([200, 137], dtype=torch.int32).cuda()
        bt2 = torch.from_numpy(b2).cuda()
        off = torch.empty((2 * 200 * 4 + 4,), device="cuda")[1:1601].view(2, 200, 4).copy_(bt2)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        run("with2d_boxes_bwd", GN.differentiable_nms_with_iou2d_batched, s2, bt2, counts=cnt, mask_group_boxes=False)
        run("with2d_matrix_bwd", GN.differentiable_nms_with_iou2d_batched, s2, bt2, counts=cnt, group_boxes=False)
        # the unaligned view: gnms_forward_with_iou2d does not run from the boxes, and the matrix path's gnms_iou2d refuses such a pointer -- in
        # both bindings alike, before anything is kept or any backward runs on it (with a forward that accepted the view, the four
        # comparisons of run() would apply as they stand)
        if str(ref["with2d_unaligned/error"]):
            with pytest.raises(GN._lib.GnmsError) as err:
                run("with2d_unaligned", GN.differentiable_nms_with_iou2d_batched, s2, off, counts=cnt, mask_group_boxes=False)
            assert "16-byte aligned" in str(err.value) and str(ref["with2d_unaligned/error"]) in str(err.value)     # (the binding's starts "GNMS: ")
        else:
            run("with2d_unaligned", GN.differentiable_nms_with_iou2d_batched, s2, off, counts=cnt, mask_group_boxes=False)
        run("with3d_unmasked", GN.differentiable_nms_with_iou3d_batched, s4, torch.from_numpy(p2).cuda(), counts=cnt, mask_group_boxes=False)


def test_n_rank_launcher_end_to_end():
    """The launcher path the 8-GPU scaling run takes, proven on this 1-GPU box: `python bench.py --gpus 2` and
    `tools/e2e_bench.py --mode train --gpus 2` start their two ranks themselves (dist.relaunch_under_torchrun -> torch.distributed.run,
    one process per rank) under GNMS_SHARE_GPU=1 (debug: both ranks on this GPU, gloo collectives).  Exactly one JSON line, n_gpus == 2,
    the per-step all-reduces verified (StepHeartbeat.check() raises otherwise and the rank exits non-zero), rc 0, no rank stuck in the
    final barrier while rank 0 measures its roofline (the timeout)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GNMS_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")

    def one_json_line(r):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:]
        return json.loads(lines[0])

    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"], env=env,
                       capture_output=True, text=True, timeout=900)
    d = one_json_line(r)
    import re
    waits = [float(x) for x in re.findall(r"rank \d+ waited ([0-9.]+) s in the final barrier", r.stderr)]
    assert len(waits) == 2 and max(waits) < 60.0, r.stderr[-2000:]          # no rank idles a minute behind rank 0's post-region work
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["scaling"] == "weak" and "debug_shared_gpu" in d
    assert "asynchronous" in d["config"]["collective"] and d["config"]["parallelism"].endswith("dp2") and d["roofline"]["frac"] > 0
    assert "cpu_baseline" not in d                                           # rank 0 at N = 1 only
    # the other box counts of north_star at this world size, every one timed by both ranks (bench.py `box_counts`)
    assert set(d["box_counts"]) == {"N256", "N1024", "N16384"} and all(v.get("value", 0) > 0 for v in d["box_counts"].values()), d["box_counts"]
    # C5's shape exactly as the driver's 8-GPU run would start it: 8 ranks x 8 images x 16384 cuboids, folded onto this GPU
    r5 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dim", "3", "--boxes", "16384", "--batch", "8", "--steps", "2",
                         "--warmup", "1", "--full"], env=dict(env, GNMS_BENCH_PREWARM="2"), capture_output=True, text=True, timeout=1500)
    d5 = one_json_line(r5)
    waits5 = [float(x) for x in re.findall(r"rank \d+ waited ([0-9.]+) s in the final barrier", r5.stderr)]
    assert len(waits5) == 8 and max(waits5) < 60.0, r5.stderr[-2000:]
    assert d5["n_gpus"] == 8 and d5["config"]["boxes_per_image"] == 16384 and d5["config"]["images_per_gpu"] == 8 and d5["value"] > 0
    assert d5["config"]["parallelism"].endswith("dp8") and "3D" in d5["config"]["workload"]
    e = one_json_line(subprocess.run([sys.executable, os.path.join(root, "tools", "e2e_bench.py"), "--mode", "train", "--gpus", "2", "--steps", "2",
                                      "--warmup", "1", "--batch", "1", "--topk", "512", "--height", "128", "--width", "320"], env=env,
                                     capture_output=True, text=True, timeout=900))
    assert e["n_gpus"] == 2 and e["value"] > 0 and "DDP" in e["config"]["parallelism"]


def test_nms_others_on_the_gpu(golden_misc):
    """lib/nms_others.py on the device (gnms_soft_nms, gnms_nms_sorted_shift): the reference's vectors (Soft-NMS methods 0/1/2 with its
    slot order, Girshick NMS with shift 1 and 0) and the pure-Python oracle on seeded inputs, float64 and float32, odd sizes; the
    caller's array stays untouched."""
    from groomed_nms_amd.nms_others import navneeth_soft_nms, girshick_nms
    from groomed_nms_amd import synthetic
    from oracle import nms_others_oracle as NO
    g = golden_misc
    for tag in ("dets40", "dets300", "dets_uni200"):
        d = g[f"{tag}/dets"]
        for thr in (0.4, 0.7):
            assert [int(i) for i in girshick_nms(d, thr)] == list(g[f"{tag}/girshick_nms_{thr}"]), (tag, thr)
            assert [int(i) for i in girshick_nms(d, thr, shift=0)] == list(g[f"{tag}/girshick_nms_shift0_{thr}"]), (tag, thr)
        for m in (0, 1, 2):
            d64 = d.astype(np.float64).copy()
            keep = navneeth_soft_nms(d64, method=m)
            assert list(keep) == list(g[f"{tag}/soft_nms_m{m}"]), (tag, m)
            assert np.array_equal(d64, d.astype(np.float64))                     # not modified (the reference rewrites its argument)
    rng = np.random.default_rng(17)
    for n in (1, 2, 63, 64, 65, 257, 1000, 2500):
        per = max(2, n // 12)
        dets = np.concatenate([np.round(synthetic.clustered_boxes_2d(rng, n, per)), synthetic.tie_free_scores(rng, n)[:, None]], 1)
        for m, kw in ((0, {}), (1, {}), (2, dict(sigma=0.3)), (1, dict(Nt=0.2, threshold=0.05, shift=0)), (2, dict(threshold=0.2))):
            want = list(NO.soft_nms(dets.astype(np.float64), method=m, **kw))
            assert list(navneeth_soft_nms(dets.astype(np.float64), method=m, **kw)) == want, (n, m, kw)
        # float32 input: fp32 geometry and stored scores; same kept SET as the fp64 oracle on these pixel-rounded boxes for hard NMS
        assert sorted(navneeth_soft_nms(dets.astype(np.float32), method=0)) == sorted(NO.soft_nms(dets.astype(np.float64), method=0)), n
        for thr, sh in ((0.5, 1), (0.3, 0), (0.7, 2)):
            d32 = dets.astype(np.float32)
            assert [int(i) for i in girshick_nms(d32, thr, shift=sh)] == [int(i) for i in NO.girshick_nms(d32, thr, shift=sh)], (n, thr, sh)
            # float64 `dets` (what the reference's own test feeds): every operation in double on the device, un-rounded boxes
            d64 = dets.astype(np.float64) + np.concatenate([rng.uniform(-0.4, 0.4, (n, 4)), np.zeros((n, 1))], 1)
            assert [int(i) for i in girshick_nms(d64, thr, shift=sh)] == [int(i) for i in NO.girshick_nms(d64, thr, shift=sh)], (n, thr, sh, "f64")
    assert list(navneeth_soft_nms(np.zeros((0, 5)))) == [] and girshick_nms(np.zeros((0, 5), np.float32), 0.5) == []


def test_lazy_index_lists(G, O):
    """Default: plain index tensors like the reference.  Opt-in (LAZY_INDEX_LISTS = True, GPU tensors in): the two index lists come
    back as LazyIndexList objects (no host sync inside differentiable_nms); on first use they are the tensors the eager convention
    returns, through every access path a caller of an NMS keep list uses -- as an index, in arithmetic, in comparisons."""
    from groomed_nms_amd import synthetic, groomed_nms as GN
    b, s = synthetic.batch_2d(5, 1, 300, "clustered", per=20)
    m = torch.from_numpy(O.iou2d(b[0], b[0])).cuda()
    st = torch.from_numpy(s[0]).cuda()
    ref = O.differentiable_nms(s[0], O.iou2d(b[0], b[0]))
    assert GN.LAZY_INDEX_LISTS is False
    v2, iv2, p2 = G.differentiable_nms(st, m)
    assert isinstance(v2, torch.Tensor) and isinstance(iv2, torch.Tensor) and v2.tolist() == list(ref["valid"])
    old = GN.LAZY_INDEX_LISTS
    try:
        GN.LAZY_INDEX_LISTS = True
        v, iv, p = G.differentiable_nms(st, m)
        assert type(v) is GN.LazyIndexList and type(iv) is GN.LazyIndexList and isinstance(p, torch.Tensor)
        assert torch.equal(v2, v.t) and torch.equal(iv2, iv.t) and torch.equal(p2, p)
        assert v.tolist() == list(ref["valid"]) and len(v) == len(ref["valid"]) and v.shape == (len(ref["valid"]),)
        assert v.device.type == "cuda" and v.dtype == torch.int64
        assert np.array_equal(np.asarray(iv), iv.cpu().numpy()) and sorted(iv.tolist()) == sorted(ref["invalid"].tolist())
        assert torch.equal(torch.sort(v)[0], torch.sort(v.t)[0]) and torch.equal(st[v.t], torch.index_select(st, 0, v))
        # the most common use of a keep list: as an index (1-D data and data with more dimensions), on both sides of an assignment
        boxes = torch.from_numpy(b[0]).cuda()
        cube = torch.arange(300 * 3 * 5, device="cuda", dtype=torch.float32).reshape(300, 3, 5)
        assert torch.equal(st[v], st[v.t]) and torch.equal(boxes[v], boxes[v.t]) and torch.equal(cube[v], cube[v.t])
        z = torch.zeros(300, device="cuda")
        z[v] = 1
        assert int(z.sum()) == len(v)
        assert torch.equal(v + 1, v.t + 1) and torch.equal(2 * v, 2 * v.t) and torch.equal(v < 7, v.t < 7) and torch.equal(v == v2, v.t == v2)
        assert not isinstance(v, torch.Tensor)                 # (which is why it is opt-in)
        vs, ivs, _ = G.differentiable_nms(torch.sort(st, descending=True)[0], m, sorting_method="soft", sorting_temperature=0.01)
        assert len(vs) + len(ivs) <= 300 and int(vs.max()) < 300            # soft sort: mapped through the hard-sort indices lazily as well
    finally:
        GN.LAZY_INDEX_LISTS = old
    # a tensor-valued threshold / temperature is re-read on every call (the params cache is keyed on converted values)
    thr = torch.tensor(0.4, device="cuda")
    a = G.differentiable_nms(st, m, nms_threshold=thr)[2]
    thr.fill_(0.9)
    c = G.differentiable_nms(st, m, nms_threshold=thr)[2]
    assert torch.equal(a, p2) and torch.equal(c, G.differentiable_nms(st, m, nms_threshold=0.9)[2]) and not torch.equal(a, c)


def test_bench_line_contract_on_a_small_problem():
    """bench.py --full end to end on a small problem (2 images x 512 boxes, a few steps): one JSON line with the driver's fields, the
    roofline object measured from the library's launch events, parity 0 against the oracle, the CPU baseline -- 2D, 3D and the
    matrix-in variant."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for extra in ([], ["--dim", "3"], ["--two-calls"], ["--graph", "--no-cpu-baseline"]):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--boxes", "512", "--batch", "2", "--steps", "4", "--warmup", "1",
                            "--cpu-seconds", "0.3", "--full", "--no-extras"] + extra, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                    "data", "config", "roofline"):
            assert key in d, (extra, key)
        assert d["n_gpus"] == 1 and d["steps"] == 4 and d["unit"] == "boxes/s" and d["dtype"] == "f32" and d["vs_baseline"] is None
        assert d["value"] > 0 and "workload" in d["config"]
        rf = d["roofline"]
        assert rf and rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and rf["kernel_ms"] > 0 and rf["kernel"]
        if "--graph" not in extra:
            assert d["parity"]["valid_index_sets_equal"] and d["parity"]["max_abs_dscore"] <= 1e-4 and d["parity"]["max_abs_dgrad_scores"] <= 1e-4
            if "--dim" not in extra:
                assert d["parity"]["max_abs_dscore"] == 0.0 and d["parity"]["max_abs_dgrad_scores"] == 0.0
            assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain bench.py run prints the headline line and nothing of --full; --dump-outputs writes the last timed step's outputs, the
    same on a second run, and equal to the CPU oracle on the bench's seeded inputs (eager entry and the replayed HIP graph)."""
    import json, os, subprocess, sys
    from groomed_nms_amd import synthetic
    from oracle import oracle as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    B, N = 2, 512

    def run(tag, extra=()):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--boxes", str(N), "--batch", str(B), "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / tag)] + list(extra), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0]), {f[:-4]: np.load(tmp_path / tag / f) for f in os.listdir(tmp_path / tag)}

    d, a = run("a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "boxes/s" and d["dtype"] == "f32"
    for key in ("parity", "cpu_baseline", "other_kind", "hip_graph_replay", "spread", "two_calls", "N256"):
        assert key not in d, key
    assert d["roofline"] is None
    assert set(a) == {"prob", "grad_scores", "order", "valid", "invalid", "num_valid", "num_invalid", "iou"}
    assert a["prob"].dtype == np.float32 and a["prob"].shape == (B, N) and a["iou"].shape == (B, N, N) and a["valid"].dtype == np.float64
    _, b = run("b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    boxes, scores = synthetic.batch_2d(1000, B, N, "uniform")
    w = np.linspace(-1.0, 2.0, N).astype(np.float32)
    _, g = run("graph", ["--graph"])
    assert set(g) == {"prob", "grad_scores", "iou"}
    for i in range(B):
        m = O.iou2d(boxes[i], boxes[i])
        ref = O.differentiable_nms(scores[i], m, grad_prob=w)
        for got in (a, g):
            assert np.array_equal(got["iou"][i], m, equal_nan=True)
            assert np.array_equal(got["prob"][i], ref["prob"]) and np.array_equal(got["grad_scores"][i], ref["grad_scores"])
        nv = int(a["num_valid"][i])
        assert set(a["valid"][i, :nv].astype(np.int64).tolist()) == set(ref["valid"].tolist())


def test_profile_hooks(G):
    """gnms_profile_events / _collect: armed, every matrix-writing launch is timed (start/stop events of hipExtLaunchKernel);
    disarmed nothing is recorded; the fill / read streams run."""
    import ctypes
    from groomed_nms_amd import _lib, overlaps, synthetic
    from groomed_nms_amd._lib import ptr, check, stream_ptr
    lib = _lib.load()
    b, _ = synthetic.batch_2d(1, 2, 1024, "clustered")
    bt = torch.from_numpy(b).cuda()

    def collect(slot):
        ms, n = ctypes.c_double(-1), ctypes.c_int(-1)
        check(lib.gnms_profile_collect(slot, ctypes.byref(ms), ctypes.byref(n)), "collect")
        return ms.value, n.value
    collect(0); collect(1)
    overlaps.iou_batched(bt)
    assert collect(0) == (0.0, 0)
    check(lib.gnms_profile_events(1), "arm")
    m = overlaps.iou_batched(bt)
    overlaps.iou_batched(bt)
    G.differentiable_nms_batched(torch.rand((2, 1024), device="cuda"), m)
    check(lib.gnms_profile_events(0), "disarm")
    ms, n = collect(0)
    assert n == 2 and 0 < ms < 50
    ms, n = collect(1)
    assert n == 1 and 0 < ms < 50
    assert lib.gnms_profile_write_kernel_name(2, 8, 4096).decode() == "tail_write_kernel"
    buf = torch.empty(1 << 20, device="cuda")
    sink = torch.zeros(4, device="cuda")
    check(lib.gnms_profile_fill(ptr(buf), buf.numel(), stream_ptr()), "fill")
    check(lib.gnms_profile_read(ptr(buf), buf.numel(), ptr(sink), stream_ptr()), "read")
    torch.cuda.synchronize()
    assert float(buf.min()) == 0.5 and float(buf.max()) == 0.5


def test_iou2d_division_paths_bit_exact(G, O):
    """The 2D tile divides without the scale / fixup steps (packed v_pk_fma_f32) where every box of the tile is in the range that
    makes them no-ops, and with the compiler's full IEEE division elsewhere (iou_tile.h).  Boxes chosen to sit on both sides of that
    predicate -- tiny and huge coordinates, coordinates just inside / outside 2^-13 and 2^20, zero-area, inverted, NaN and Inf boxes,
    denormal extents -- mixed into ordinary pixel boxes: every entry must equal the oracle's IEEE division bit for bit, through
    gnms_iou2d AND through the matrix the fused launch writes (staged persistent writers, N = 2048), whose layer output must also
    match the oracle run on that matrix."""
    from groomed_nms_amd import overlaps, synthetic
    rng = np.random.default_rng(77)

    def adversarial(n):
        b = synthetic.clustered_boxes_2d(rng, n, 16)
        specials = [
            (0.0, 0.0, 0.0, 0.0), (5.0, 5.0, 5.0, 9.0), (9.0, 3.0, 2.0, 8.0),                       # zero-area, degenerate, inverted
            (1e-6, 1e-6, 3e-6, 4e-6), (1e-20, 1e-20, 2e-20, 3e-20), (1e-39, 0.0, 3e-39, 2e-39),        # tiny / denormal
            (2.0 ** -13, 2.0 ** -13, 2.0 ** -12, 2.0 ** -12), (2.0 ** -14, 0.0, 2.0 ** -12, 1.0),      # the predicate's lower edge
            (0.0, 0.0, 2.0 ** 20 - 1.0, 2.0 ** 19), (0.0, 0.0, 2.0 ** 20, 2.0 ** 20),                  # ... and upper edge
            (1e7, 1e7, 3e7, 2e7), (1e18, 1e18, 3e18, 3e18), (-1e30, -1e30, 1e30, 1e30),                # huge (areas overflow towards inf)
            (float("nan"), 0.0, 1.0, 1.0), (0.0, 0.0, float("inf"), 1.0), (-float("inf"), 0.0, 0.0, 1.0),
            (100.0, 100.0, 100.00001, 100.00001), (-50.0, -50.0, 50.0, 50.0),
        ]
        where = rng.choice(n, size=min(n // 3, 8 * len(specials)), replace=False)
        for i, k in enumerate(where):
            b[k] = specials[i % len(specials)]
        return b.astype(np.float32)

    for n in (64, 300, 1024):
        a, b = adversarial(n), adversarial(n + 13)
        got = overlaps.iou(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        assert np.array_equal(got, O.iou2d(a, b), equal_nan=True), n
    # boxes at the edges of what the predicate admits (so the tiles DO take the plain division): zero-area boxes (0 / 0 -> NaN),
    # coordinates of exactly 2^-13 and just under 2^20, sub-ulp extents next to large coordinates, a box covering everything
    edge = [(0.0, 0.0, 0.0, 0.0), (5.0, 5.0, 5.0, 9.0), (2.0 ** -13, 2.0 ** -13, 2.0 ** -12, 2.0 ** -12), (0.0, 0.0, 2.0 ** -13, 2.0 ** -13),
            (0.0, 0.0, 2.0 ** 20 - 1.0, 2.0 ** 19), (-(2.0 ** 20 - 1.0), -(2.0 ** 20 - 1.0), 2.0 ** 20 - 1.0, 2.0 ** 20 - 1.0),
            (100.0, 100.0, 100.00001, 100.00001), (1000000.0, 1000000.0, 1000000.0625, 1000000.0625), (2.0 ** -13, 0.0, 2.0 ** 19, 2.0 ** -13)]
    for n in (256, 777):
        a = synthetic.clustered_boxes_2d(rng, n, 16).astype(np.float32)
        for i, k in enumerate(rng.choice(n, size=n // 4, replace=False)):
            a[k] = edge[i % len(edge)]
        got = overlaps.iou(torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda()).cpu().numpy()
        assert np.array_equal(got, O.iou2d(a, a), equal_nan=True), n
    # through the fused launch: two images, one ordinary (every tile plain), one adversarial (tiles on both paths)
    N = 2048
    boxes = np.stack([synthetic.clustered_boxes_2d(rng, N, 24).astype(np.float32), adversarial(N)])
    boxes[1, ::2] = np.where(np.isfinite(boxes[1, ::2]), boxes[1, ::2], 1.0)                        # keep half of the weird boxes finite
    scores = rng.random((2, N), dtype=np.float32)
    st = torch.from_numpy(scores).cuda().requires_grad_(True)
    out = G.differentiable_nms_with_iou2d_batched(st, torch.from_numpy(boxes).cuda())
    for i in range(2):
        want = O.iou2d(boxes[i], boxes[i])
        got = out[6][i].cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), i
    ref = O.differentiable_nms(scores[0], O.iou2d(boxes[0], boxes[0]))
    assert np.array_equal(out[0][0].detach().cpu().numpy(), ref["prob"])


def test_iou2d_large_rectangular_through_the_persistent_writers(G, O):
    """gnms_iou2d routes large matrices (N > 4096, N % 4 == 0, enough 8-row units) through write_staged_kernel (the smaller ones here
    take the 64-row tiles): persistent workgroups, column
    groups staged in LDS, rows and columns from DIFFERENT box sets, M != N, ragged last column tile, balanced column groups (N = 4100:
    17 wave tiles = 9 + 8), a leading dimension wider than N.  Every entry equals the oracle's; the rows past M and the padding
    columns of a wider `ld` stay untouched."""
    from groomed_nms_amd import _lib, synthetic
    from groomed_nms_amd._lib import ptr, check, stream_ptr
    lib = _lib.load()
    rng = np.random.default_rng(123)
    for B, M, N, ld in ((8, 1100, 2052, 2052), (3, 3000, 4100, 4100), (2, 4500, 1024, 1040), (2, 4000, 4104, 4112), (1, 9000, 8200, 8200)):
        a = np.stack([synthetic.clustered_boxes_2d(rng, M, 16) for _ in range(B)]).astype(np.float32)
        b = np.stack([synthetic.uniform_boxes_2d(rng, N) for _ in range(B)]).astype(np.float32)
        out = torch.full((B, M + 3, ld), -7.0, device="cuda")
        # (image stride M * ld: the entry's layout; the 3 spare rows sit behind the last image)
        flat = out.view(-1)[: B * M * ld].view(B, M, ld)
        at, bt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        check(lib.gnms_iou2d(ptr(at), ptr(bt), B, M, N, ptr(flat), ld, stream_ptr()), "gnms_iou2d")
        torch.cuda.synchronize()
        got = flat.cpu().numpy()
        for i in range(B if M * N < 3e7 else 1):
            assert np.array_equal(got[i, :, :N], O.iou2d(a[i], b[i]), equal_nan=True), (B, M, N, i)
        if ld > N:
            assert float(got[:, :, N:].min()) == -7.0 and float(got[:, :, N:].max()) == -7.0
        assert float(out.view(-1)[B * M * ld:].min()) == -7.0


def test_one_call_matrix_with_a_sliver_of_a_last_column_tile(G, O):
    """N = 256 k + 4: the last wave tile of a row band has ONE valid lane.  The staged writers broadcast a tile's rows out of the first
    lanes' registers, so such a tile must not take the path on which the other lanes sit the stores out (iou_tile.h); the matrix of the
    one-call entry equals the oracle's everywhere, through the fused launch (N = 1284, 2052) and the large-image launch (N = 4100)."""
    from groomed_nms_amd import synthetic
    for B, N in ((2, 1284), (2, 2052), (1, 4100)):
        boxes, scores = synthetic.batch_2d(31, B, N, "clustered")
        out = G.differentiable_nms_with_iou2d_batched(torch.from_numpy(scores).cuda(), torch.from_numpy(boxes).cuda())
        for i in range(B):
            want = O.iou2d(boxes[i], boxes[i])
            assert np.array_equal(out[6][i].cpu().numpy(), want, equal_nan=True), (N, i)
            ref = O.differentiable_nms(scores[i], want)
            assert np.array_equal(out[0][i].cpu().numpy(), ref["prob"]), (N, i)


def test_classic_nms_beyond_the_layer_limit(G, O):
    """`_nms` on more boxes than the layer's 16384 (the reference's inference path hands gpu_nms every anchor, lib/rpn_util.py:1268):
    round 6 works in chunks of 16384 -- what the boxes kept so far suppress in the chunk (classic_ext_kernel), the chunk's own bit matrix, the
    layer's scan with those boxes removed from the start, the kept boxes appended -- kept indices identical to the oracle's; sizes around the
    64-box block edge and the chunk edge, one / two / three chunks, few clusters (every later chunk almost wholly suppressed by the first
    chunk's boxes: the kept list stays tiny) and many (it grows to thousands); the +1-pixel rule and the <= rule of girshick_nms; beyond
    262144 boxes it refuses."""
    from groomed_nms_amd import synthetic, _lib, nms_others
    from groomed_nms_amd.nms import gpu_nms
    rng = np.random.default_rng(17)
    for n, per in ((16385, 8), (20000, 24), (33000, 3), (32768, 4000), (32769, 40), (49153, 16), (40000, 20000)):
        dets = np.concatenate([synthetic.clustered_boxes_2d(rng, n, per), synthetic.tie_free_scores(rng, n)[:, None]], 1).astype(np.float32)
        got = [int(i) for i in gpu_nms(dets, 0.5)]
        assert got == O.classic_nms(dets, 0.5, rule="gpu"), n
        if n <= 20000:                                     # boxes that arrive sorted (both call sites of the reference): the wrapper skips sort + gather
            sd = dets[np.argsort(-dets[:, 4], kind="stable")]
            assert [int(i) for i in gpu_nms(sd, 0.5)] == O.classic_nms(sd, 0.5, rule="gpu"), ("sorted", n)
            sd[7, 4] = sd[6, 4]                            # ... and a tie takes the reference's argsort()[::-1] again
            assert [int(i) for i in gpu_nms(sd, 0.5)] == O.classic_nms(sd, 0.5, rule="gpu"), ("tie", n)
    dets = np.concatenate([synthetic.clustered_boxes_2d(rng, 20000, 12), synthetic.tie_free_scores(rng, 20000)[:, None]], 1).astype(np.float32)
    from oracle import nms_others_oracle as NO
    assert [int(i) for i in nms_others.girshick_nms(dets, 0.45)] == [int(i) for i in NO.girshick_nms(dets, 0.45)], "girshick_nms (<= rule), float32 boxes in chunks"
    with pytest.raises(_lib.GnmsError):
        gpu_nms(np.zeros((262145, 5), np.float32), 0.5)


def test_select_topk_among_all_anchors(G):
    """gnms_select_topk with more candidates than one workgroup sorts (the reference's inference path selects among ALL anchors,
    lib/rpn_util.py:1258-1266): the radix pre-selection leaves exactly what the stable descending sort would -- scores with many exact
    ties and NaNs, with and without a candidate list and ragged candidate counts, K at and around the number of distinct maxima."""
    from groomed_nms_amd import proposals as PR
    from oracle import proposals_oracle as PO
    rng = np.random.default_rng(91)
    B, A = 3, 126720
    sc = rng.random((B, A), dtype=np.float32)
    sc[1] = np.round(sc[1] * 50) / 50                                     # 51 distinct values: thousands of ties at every threshold
    sc[2, rng.choice(A, 1000, replace=False)] = np.nan
    boxes = rng.random((B, A, 4), dtype=np.float32)
    st, bt = torch.from_numpy(sc).cuda(), torch.from_numpy(boxes).cuda()
    for K in (1, 500, 4096, 16384):
        idx, num, ssel, bsel = PR.select_topk(st, K, boxes=bt)
        for b in range(B):
            want = PO.select_topk(sc[b], None, K)
            assert int(num[b]) == len(want) and idx[b, :len(want)].cpu().tolist() == want.tolist(), (K, b)
            assert np.array_equal(ssel[b, :len(want)].cpu().numpy(), sc[b][want], equal_nan=True)
            assert np.array_equal(bsel[b, :len(want)].cpu().numpy(), boxes[b][want])
    # a candidate list longer than the in-LDS sort takes, ragged counts (one image below K, one below the limit)
    F = 40000
    cand = np.stack([rng.permutation(A)[:F] for _ in range(B)]).astype(np.int32)
    counts = np.array([F, 300, 17000], np.int32)
    K = 1000
    idx, num, ssel, _ = PR.select_topk(st, K, torch.from_numpy(cand).cuda(), torch.from_numpy(counts).cuda())
    for b in range(B):
        want = PO.select_topk(sc[b], cand[b, :counts[b]], K)
        assert int(num[b]) == len(want) and idx[b, :len(want)].cpu().tolist() == want.tolist(), b
        assert (idx[b, len(want):] == -1).all()
    # round 5, the cooperative launch (several workgroups per image from 4096 candidates on): candidate counts on both sides of its chunk
    # (8192) and run (1024) boundaries, K above the count, ALL scores equal (every key ties at the threshold: candidate order decides),
    # batches of one image and of sixteen
    for Bq, Aq, K in ((1, 126720, 4096), (16, 20000, 3000), (2, 8193, 8192), (3, 5000, 6000), (1, 4097, 1025)):
        sq = rng.random((Bq, Aq), dtype=np.float32)
        sq[0, : Aq // 2] = 0.5                                             # half of image 0 ties
        if Bq > 1:
            sq[1] = 0.25                                                   # image 1: one value
        bq = rng.random((Bq, Aq, 4), dtype=np.float32)
        cq = rng.integers(1, Aq + 1, size=Bq).astype(np.int32)
        cq[0] = Aq
        idx, num, ssel, bsel = PR.select_topk(torch.from_numpy(sq).cuda(), K, torch.arange(Aq, dtype=torch.int32).repeat(Bq, 1).cuda(),
                                              torch.from_numpy(cq).cuda(), torch.from_numpy(bq).cuda())
        for b in range(Bq):
            want = PO.select_topk(sq[b], np.arange(cq[b]), K)
            assert int(num[b]) == len(want) and idx[b, :len(want)].cpu().tolist() == want.tolist(), (Bq, Aq, K, b)
            assert (idx[b, len(want):] == -1).all() and (ssel[b, len(want):] == 0).all()
            assert np.array_equal(ssel[b, :len(want)].cpu().numpy(), sq[b][want]) and np.array_equal(bsel[b, :len(want)].cpu().numpy(), bq[b][want])
    # two host threads on two streams at once: the cooperative launches must not wait for each other's workgroups for ever
    import threading
    big = torch.from_numpy(rng.random((12, 126720), dtype=np.float32)).cuda()          # 12 x 16 workgroups: three quarters of the machine per launch
    want0 = PO.select_topk(big[0].cpu().numpy(), None, 4096)
    errs = []

    def worker():
        try:
            st_ = torch.cuda.Stream()
            with torch.cuda.stream(st_):
                for _ in range(20):
                    idx_, _, _, _ = PR.select_topk(big, 4096)
                st_.synchronize()
            assert idx_[0].cpu().tolist() == want0.tolist()
        except Exception as e:                                             # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=worker) for _ in range(2)]
    [t_.start() for t_ in th]
    [t_.join(timeout=120) for t_ in th]
    assert not any(t_.is_alive() for t_ in th), "concurrent cooperative top-K launches hang"
    assert not errs, errs


def test_self_iou_in_the_writers_geometry_and_negative_zero(G, O):
    """gnms_iou2d(boxes, boxes) with enough 8-row units runs the staged writers as a launch of their own (iou2d_self_kernel: claimed
    units, columns cached in registers, the packed tile body); the same boxes through a second buffer (a != b) take iou2d_kernel.  Both
    must equal the oracle's IEEE values bit for bit -- on ordinary boxes (every image plain), on a batch with one adversarial image
    (that image takes the general body) and with NEGATIVE-ZERO coordinates, which the plain body must never see (a difference could
    then be -0 where the reference's min - max is +0): box_divides_plainly rejects them."""
    from groomed_nms_amd import overlaps, synthetic
    rng = np.random.default_rng(404)
    B, N = 8, 2048                                              # 8 * 256 units = the threshold of the self path
    boxes = np.stack([synthetic.clustered_boxes_2d(rng, N, 32) if i % 2 else synthetic.uniform_boxes_2d(rng, N) for i in range(B)]).astype(np.float32)
    boxes[3, 5] = (0.0, 0.0, 0.0, 0.0)
    boxes[3, 77] = (float("nan"), 1.0, 2.0, 3.0)               # image 3: not plain
    boxes[5, 10] = (-0.0, 3.0, 40.0, 50.0)                      # image 5: a negative zero (x1 = -0 touches boxes that start at +0)
    boxes[5, 11] = (0.0, -0.0, 25.0, 30.0)
    boxes[5, 12] = (0.0, 0.0, 25.0, 3.0)
    bt = torch.from_numpy(boxes).cuda()
    same = overlaps.iou_batched(bt, bt).cpu().numpy()
    other = overlaps.iou_batched(bt, bt.clone()).cpu().numpy()
    for i in range(B):
        want = O.iou2d(boxes[i], boxes[i])
        assert np.array_equal(same[i], want, equal_nan=True), i
        assert np.array_equal(other[i], want, equal_nan=True), i
    # the same images through the layer's launch (tail_write_kernel's writers) and its bit matrix (packed body + sign decision)
    scores = rng.random((B, N), dtype=np.float32)
    out = G.differentiable_nms_with_iou2d_batched(torch.from_numpy(scores).cuda(), bt)
    for i in (0, 3, 5):
        assert np.array_equal(out[6][i].cpu().numpy(), O.iou2d(boxes[i], boxes[i]), equal_nan=True), i
        ref = O.differentiable_nms(scores[i], O.iou2d(boxes[i], boxes[i]))
        assert np.array_equal(out[0][i].cpu().numpy(), ref["prob"], equal_nan=True), i


def test_leader_scan_across_workgroups(G, O):
    """Round 4: the leader scan of a symmetric bit matrix runs on one workgroup per super-block (1024 ranks), the masks handed down
    the chain as epoch-tagged granules.  Everything the hand-off could get wrong, against the oracle: box counts on both sides of
    super-block boundaries with ragged images (fewer super-blocks than the launch provides), both entries (bits from the boxes inside
    the write launch / from the matrix behind the symmetry check), the SAME workspace and buffers reused back to back and replayed from a
    captured graph (stale granules of earlier calls must never match: the call counter lives in the workspace and advances inside the
    captured sort kernels), and batches with more chain workgroups than CUs (a workgroup may only wait for ones dispatched before it)."""
    import ctypes
    from groomed_nms_amd import synthetic, overlaps, _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, check
    for B, N, kind, counts in ((3, 1025, "uniform", [1025, 1024, 7]), (2, 2049, "clustered", [2049, 1100]), (3, 4096, "uniform", [4096, 3073, 3072]),
                               (2, 6000, "uniform", [6000, 5121]), (2, 9000, "clustered", [9000, 8193])):
        boxes, scores = synthetic.batch_2d(40 + N, B, N, kind)
        bt, st = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        ct = torch.tensor(counts, dtype=torch.int32).cuda()
        one = G.differentiable_nms_with_iou2d_batched(st, bt, counts=ct)
        two = G.differentiable_nms_batched(st, overlaps.iou_batched(bt), counts=ct)
        for b in range(B):
            n = counts[b]
            ref = O.differentiable_nms(scores[b][:n], O.iou2d(boxes[b][:n], boxes[b][:n]))
            for tag, out in (("one-call", one), ("matrix-in", two)):
                assert np.array_equal(out[0][b, :n].cpu().numpy(), ref["prob"], equal_nan=True), (N, b, tag)
                assert out[2][b, :int(out[4][b])].tolist() == list(ref["valid"]), (N, b, tag)
    # one workspace, eager twice, then captured and replayed on new inputs
    lib = _lib.load()
    B, N = 3, 4096
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    dev = torch.device("cuda")
    bx, sc = torch.empty((B, N, 4), device=dev), torch.empty((B, N), device=dev)
    iou, prob = torch.empty((B, N, N), device=dev), torch.empty((B, N), device=dev)
    ws = torch.empty(lib.gnms_workspace_bytes(B, N, ctypes.byref(P)), dtype=torch.uint8, device=dev)
    ws.fill_(0xA5)                                                       # (a recycled allocation, not fresh zeros)

    def run(stream):
        check(lib.gnms_forward_with_iou2d(ptr(bx), ptr(sc), B, N, N, None, ctypes.byref(P), ptr(iou), ptr(prob), None, None, None, None, None,
                                          ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)), "fwd")

    def load(seed):
        b, s = synthetic.batch_2d(seed, B, N, "uniform")
        bx.copy_(torch.from_numpy(b)); sc.copy_(torch.from_numpy(s))
        return b, s

    def check_against_oracle(b, s, what):
        torch.cuda.synchronize()
        for i in range(B):
            ref = O.differentiable_nms(s[i], O.iou2d(b[i], b[i]))
            assert np.array_equal(prob[i].cpu().numpy(), ref["prob"]), (what, i)
    for seed in (1, 2):
        b, s = load(seed)
        run(torch.cuda.current_stream())
        check_against_oracle(b, s, "eager %d" % seed)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream())
    for seed in (3, 4, 5):
        b, s = load(seed)
        graph.replay()
        check_against_oracle(b, s, "replay %d" % seed)
    # more chain workgroups than CUs: 160 images x 2 super-blocks (and the writers behind them)
    B, N = 160, 2048
    boxes, scores = synthetic.batch_2d(77, 4, N, "uniform")
    bt = torch.from_numpy(np.tile(boxes, (B // 4, 1, 1))).cuda()
    stt = torch.from_numpy(np.tile(scores, (B // 4, 1))).cuda()
    out = G.differentiable_nms_with_iou2d_batched(stt, bt)
    torch.cuda.synchronize()
    for b in range(4):
        ref = O.differentiable_nms(scores[b], O.iou2d(boxes[b], boxes[b]))
        for rep in (b, b + 4, B - 4 + b):
            assert np.array_equal(out[0][rep].cpu().numpy(), ref["prob"]), rep
    # the same batch through the matrix-in layer (round 5: symmetry checkers in FRONT of 480 chain / CSR workgroups that wait for them)
    two = G.differentiable_nms_batched(stt, out[6])
    torch.cuda.synchronize()
    assert torch.equal(two[0], out[0]) and torch.equal(two[2], out[2]) and torch.equal(two[4], out[4])


def test_library_switches():
    """The environment switches the shipped library still reads (four since round 6), each against the default run
    of the same inputs: GNMS_FAST_TAIL=0 (round 5: K5 proper -- the sort of the groups -- instead of the fast tail; probabilities, lists AND
    gradients, i.e. the groups' runs the backward reads, must be the same bit for bit), GNMS_MATRIX_SYM=0 (matrix-in layer: the general scan
    also for symmetric matrices), GNMS_TRACE_LAUNCH=1 (developer: launch sites printed, device synchronised behind each) and
    GNMS_ONE_LAUNCH=0 (round 6: small images in three launches; its own cases: test_one_launch_against_three_launches)."""
    code = """
import sys, numpy as np, torch
import groomed_nms_amd as G
from groomed_nms_amd import synthetic, overlaps
out = {}
b, s = synthetic.batch_2d(7, 2, 4096, "uniform")
bt, st = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
st.requires_grad_(True)
wt = torch.linspace(-1.0, 2.0, 4096, device="cuda").repeat(2, 1)
o = G.differentiable_nms_with_iou2d_batched(st, bt)
out["one_prob"], out["one_valid"], out["one_iou_sum"] = o[0].detach().cpu().numpy(), o[2].cpu().numpy(), o[6].double().sum().cpu().numpy()
(o[0] * wt).sum().backward()
out["one_grad"] = st.grad.cpu().numpy().copy()
st.grad = None
m = G.differentiable_nms_batched(st, overlaps.iou_batched(bt))
out["two_prob"], out["two_valid"] = m[0].detach().cpu().numpy(), m[2].cpu().numpy()
(m[0] * wt).sum().backward()
out["two_grad"] = st.grad.cpu().numpy().copy()
for gs in (2, 30):            # groups above the cap: the fast tail's verdict is "slow"
    bc, sc_ = synthetic.batch_2d(11, 2, 3000, "clustered")
    sct = torch.from_numpy(sc_).cuda().requires_grad_(True)
    o = G.differentiable_nms_with_iou2d_batched(sct, torch.from_numpy(bc).cuda(), group_size=gs)
    (o[0] * wt[:, :3000]).sum().backward()
    out["cap%d_prob" % gs], out["cap%d_valid" % gs], out["cap%d_grad" % gs] = o[0].detach().cpu().numpy(), o[2].cpu().numpy(), sct.grad.cpu().numpy().copy()
b, s = synthetic.batch_2d(8, 2, 8192, "clustered")
bt, st = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
o = G.differentiable_nms_with_iou2d_batched(st, bt)
out["big_prob"], out["big_valid"], out["big_iou_sum"] = o[0].cpu().numpy(), o[2].cpu().numpy(), o[6].double().sum().cpu().numpy()
p3, s3 = synthetic.batch_3d(9, 2, 6144, clustered=True)
o = G.differentiable_nms_with_iou3d_batched(torch.from_numpy(s3).cuda(), torch.from_numpy(p3).cuda())
out["d3_prob"], out["d3_valid"] = o[0].cpu().numpy(), o[2].cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print("ok")
"""
    runs = {}
    for tag, env in (("default", {}), ("general_scan", {"GNMS_MATRIX_SYM": "0"}), ("trace", {"GNMS_TRACE_LAUNCH": "1"}), ("k5_proper", {"GNMS_FAST_TAIL": "0"}),
                     ("three_launches", {"GNMS_ONE_LAUNCH": "0"})):
        path = "/tmp/gnms_switch_%s.npz" % tag
        r = _run_py(code, env, argv=(path,))
        assert r.returncode == 0 and "ok" in r.stdout, (tag, r.stderr[-2000:])
        if tag == "trace":
            assert "[gnms launch]" in r.stderr
        runs[tag] = np.load(path)
    for tag, d in runs.items():
        for k in runs["default"].files:
            assert np.array_equal(d[k], runs["default"][k], equal_nan=True), (tag, k)


def test_matrix_in_layer_detects_symmetry(G, O):
    """differentiable_nms(scores, iou) cannot know that its matrix is iou(boxes, boxes); since round 3 it finds out on the device
    (bitmask_kernel stores the rows of the bit matrix in full, wsym_check_kernel compares its 64 x 64 blocks with their transposes)
    and lets the pulling, attributing scan run where the thresholded matrix is symmetric and sparse.  Every variant must equal the
    oracle: a symmetric sparse matrix (uniform boxes: the new path), a symmetric dense one (clustered boxes: skipped by the density
    gate), the same matrices with ONE entry pushed across the threshold on one side only (asymmetric by a single bit: general
    scan), and a matrix of random numbers; N on both sides of the one-launch tail (2048) and ragged."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(2718)
    for N, kind in ((1000, "uniform"), (2048, "uniform"), (4096, "uniform"), (4096, "clustered")):
        boxes = (synthetic.uniform_boxes_2d(rng, N) if kind == "uniform" else synthetic.clustered_boxes_2d(rng, N, 32)).astype(np.float32)
        scores = rng.random(N, dtype=np.float32)
        sym = O.iou2d(boxes, boxes)
        asym = sym.copy()
        i, j = np.argwhere((sym > 0.45) & (np.arange(N)[:, None] != np.arange(N)[None, :]))[0]
        asym[i, j] = 0.1                                          # (i, j) drops below the threshold, (j, i) stays above it
        rnd = rng.random((N, N), dtype=np.float32) * 0.6
        mats = np.stack([sym, asym, rnd])
        sc = np.stack([scores] * 3)
        st = torch.from_numpy(sc).cuda().requires_grad_(True)
        prob, order, valid, invalid, nv, ni = G.differentiable_nms_batched(st, torch.from_numpy(mats).cuda())
        w = torch.rand((3, N), device="cuda")
        (prob * w).sum().backward()
        for b in range(3):
            ref = O.differentiable_nms(sc[b], mats[b], grad_prob=w[b].cpu().numpy())
            assert np.array_equal(prob[b].detach().cpu().numpy(), ref["prob"]), (N, kind, b)
            assert valid[b, :int(nv[b])].tolist() == list(ref["valid"]), (N, kind, b)
            assert invalid[b, :int(ni[b])].tolist() == list(ref["invalid"]), (N, kind, b)
            assert np.array_equal(st.grad[b].cpu().numpy(), ref["grad_scores"]), (N, kind, b)


@pytest.mark.gpu
def test_recycled_workspace_bytes(G, O):
    """The workspace and the matrix are caller memory with ANY previous contents -- the torch allocator hands the layer the bytes of freed
    index lists (all 0xff: the -1 padding), of old matrices, of old workspaces.  Every entry must produce, bit for bit, what it produces on
    zeroed memory.  (Round 4b: a workspace whose call counter read 0xffffffff wrapped to 0, the tag of a freshly cleared hand-off granule,
    and the leader scan of the matrix-in layer ran ahead of its predecessors -- found by test_fuzz_layer_against_oracle when the layout moved.)"""
    import ctypes
    from groomed_nms_amd import synthetic, _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, check
    lib = _lib.load()
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    dev = torch.device("cuda")

    def fills(nbytes):
        yield "zero", (lambda t: t.zero_())
        yield "ff", (lambda t: t.fill_(0xFF))
        yield "a5", (lambda t: t.fill_(0xA5))
        yield "7f", (lambda t: t.fill_(0x7F))
        yield "rand", (lambda t: t.copy_(torch.randint(0, 256, (t.numel(),), dtype=torch.uint8, device=dev)))

    for dim, B, N, counts, mode in ((2, 2, 300, [300, 77], "gm"), (2, 2, 2300, [2300, 1331], "gm"), (2, 2, 4096, [4096, 3000], "gm"), (2, 1, 6000, [6000], "gm"),
                                    (3, 2, 700, [700, 130], "gm"), (3, 2, 2300, [2300, 1331], "gm"), (3, 1, 5000, [5000], "gm"),
                                    (2, 2, 1500, [1500, 700], "gu"), (2, 2, 1500, [1500, 700], "un"), (3, 2, 1500, [1500, 700], "gu"), (2, 2, 200, [200, 64], "un")):
        P.group_boxes, P.mask_group_boxes = (1, 1) if mode == "gm" else ((1, 0) if mode == "gu" else (0, 0))   # grouped + masked / grouped / ungrouped
        if dim == 2:
            src_np, sc_np = synthetic.batch_2d(7 + N, B, N, "clustered", per=40)
        else:
            src_np, sc_np = synthetic.batch_3d(7 + N, B, N, clustered=True, per=40)
        src, sc = torch.from_numpy(src_np).to(dev), torch.from_numpy(sc_np).to(dev)
        ct = torch.tensor(counts, dtype=torch.int32, device=dev)
        nbytes = lib.gnms_workspace_bytes(B, N, ctypes.byref(P))
        ref = {}
        for name, fill in fills(nbytes):
            for entry in ("one_call", "matrix_in"):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                fill(ws)
                iou = torch.empty((B, N, N), device=dev)
                fill(iou.view(torch.uint8).view(-1))
                prob = torch.empty((B, N), device=dev)
                valid = torch.empty((B, N), dtype=torch.int64, device=dev)
                invalid = torch.empty((B, N), dtype=torch.int64, device=dev)
                nv, ni = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
                grad = torch.empty((B, N), device=dev)
                wgt = torch.linspace(-1.0, 2.0, N, device=dev).repeat(B, 1).contiguous()
                if entry == "one_call":
                    fwd = lib.gnms_forward_with_iou2d if dim == 2 else lib.gnms_forward_with_iou3d
                    check(fwd(ptr(src), ptr(sc), B, N, N, ptr(ct), ctypes.byref(P), ptr(iou), ptr(prob), None, ptr(valid), ptr(invalid), ptr(nv), ptr(ni),
                              ptr(ws), nbytes, None), "fwd")
                else:
                    if dim == 2:
                        check(lib.gnms_iou2d(ptr(src), ptr(src), B, N, N, ptr(iou), N, None), "iou2d")
                    else:
                        check(lib.gnms_nms_overlap3d_from_params(ptr(src), B, N, float(P.nms_threshold), ptr(iou), N, None), "overlap3d")
                    check(lib.gnms_forward(ptr(sc), ptr(iou), B, N, N, ptr(ct), ctypes.byref(P), ptr(prob), None, ptr(valid), ptr(invalid), ptr(nv), ptr(ni),
                                           ptr(ws), nbytes, None), "fwd")
                check(lib.gnms_backward(ptr(wgt), ptr(sc), ptr(iou), B, N, N, ptr(ct), ctypes.byref(P), ptr(grad), None, ptr(ws), nbytes, None), "bwd")
                torch.cuda.synchronize()
                got = []
                for b in range(B):
                    n = counts[b]
                    got.append((prob[b, :n].cpu().numpy().copy(), grad[b, :n].cpu().numpy().copy(), valid[b, :int(nv[b])].cpu().numpy().copy(),
                                invalid[b, :int(ni[b])].cpu().numpy().copy()))
                if name == "zero":
                    ref[entry] = got
                    continue
                for b in range(B):
                    for a, r in zip(got[b], ref[entry][b]):
                        assert np.array_equal(a, r, equal_nan=True), (dim, N, mode, entry, name, b)
        # and the two entries agree on the probabilities (2D: bit for bit; 3D: the matrix-in layer thresholds the very matrix the one-call entry wrote)
        for b in range(B):
            assert np.array_equal(ref["one_call"][b][0], ref["matrix_in"][b][0], equal_nan=True), (dim, N, mode, b)


@pytest.mark.gpu
def test_non_default_modes_one_call_against_matrix_in_and_oracle(G, O):
    """Round 4b: behind gnms_forward_with_iou2d the grouped unmasked mode runs its group structure inside the write launch (N <= 4096), solves
    its groups one wave / one workgroup each from the BOXES (forward and backward) and the ungrouped mode builds its pruned triangular matrix
    from the boxes.  Against the matrix-in entry (bit for bit: the same solves on bit-identical overlaps) and the oracle (TOL): group sizes on
    both sides of the wave path's 32 and the tile's 128 members, ragged counts, N on both sides of 1024 / 4096 for the unmasked mode; the
    ungrouped mode at sizes that are not multiples of 16 or 64 (its solution is ill-conditioned beyond a few hundred boxes)."""
    from groomed_nms_amd import synthetic, overlaps
    rng = np.random.default_rng(77)
    cases = [(2, 257, 8, dict(mask_group_boxes=False), [257, 100]), (2, 1500, 40, dict(mask_group_boxes=False), [1500, 1111]),
             (2, 1500, 150, dict(mask_group_boxes=False, group_size=300), [1500, 900]), (1, 4096, 64, dict(mask_group_boxes=False), [4096]),
             (2, 5000, 20, dict(mask_group_boxes=False, group_size=3), [5000, 4097]),
             (2, 300, 150, dict(mask_group_boxes=False, pruning_method="sigmoidal", temperature=0.3), [300, 299]),
             (2, 191, 8, dict(group_boxes=False), [191, 65]), (1, 100, 4, dict(group_boxes=False), [100]), (2, 272, 8, dict(group_boxes=False), [272, 17])]
    for B, N, per, kw, counts in cases:
        boxes, scores = synthetic.batch_2d(int(rng.integers(1 << 30)), B, N, "clustered", per=per)
        w = rng.uniform(-1, 2, (B, N)).astype(np.float32)
        bt, wt = torch.from_numpy(boxes).cuda(), torch.from_numpy(w).cuda()
        ct = torch.tensor(counts, dtype=torch.int32).cuda()
        s1 = torch.from_numpy(scores).cuda().requires_grad_(True)
        s2 = torch.from_numpy(scores).cuda().requires_grad_(True)
        one = G.differentiable_nms_with_iou2d_batched(s1, bt, counts=ct, **kw)
        two = G.differentiable_nms_batched(s2, overlaps.iou_batched(bt), counts=ct, **kw)
        (one[0] * wt).sum().backward()
        (two[0] * wt).sum().backward()
        tag = (B, N, per, kw)
        for a, b2 in zip(one[:6], two):
            assert torch.equal(a, b2) or torch.allclose(a, b2, atol=0, rtol=0, equal_nan=True), tag
        assert torch.equal(s1.grad, s2.grad), tag
        if N > 2000 and not kw.get("group_boxes", True):
            continue
        for b in range(B):
            n = counts[b]
            ref = O.differentiable_nms(scores[b, :n], O.iou2d(boxes[b, :n], boxes[b, :n]), grad_prob=w[b, :n], **kw)
            np.testing.assert_allclose(one[0][b, :n].detach().cpu().numpy(), ref["prob"], atol=TOL, err_msg=str(tag))
            np.testing.assert_allclose(s1.grad[b, :n].cpu().numpy(), ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=str(tag))


@pytest.mark.gpu
def test_fuzz_3d_one_call_against_its_own_matrix(G):
    """Seeded fuzz of the 3D one-call entry (records -> column sort by (z band, x centre) -> slot-culled bit matrix -> chain beside the
    symmetric writers): the layer it runs from the RECORDS must agree, bit for bit, with the matrix-in layer run on the very matrix it wrote
    -- every cull of the bit-matrix kernel is then proven conservative and every evaluated decision equal to thresholding the entry.
    Box counts on both sides of 64 / 256 / 1024 / 4096, ragged counts, thresholds on both sides of the cull's 0.01 limit, scenes that are
    flat in z (one band gets everything), clustered and uniform, and cuboids with zero / negative / NaN extents (never culled, exact order)."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(20260929)
    for trial in range(100):
        B = int(rng.integers(1, 4))
        N = int(rng.choice([3, 63, 64, 65, 130, 257, 520, 1024, 1025, 1500, 2300, 4096, 4100, 5000]))
        clustered = bool(rng.uniform() < 0.5)
        par, scores = synthetic.batch_3d(int(rng.integers(1 << 30)), B, N, clustered=clustered, per=int(rng.choice([4, 32, 120])))
        style = rng.uniform()
        if style < 0.2:
            par[:, :, 2] = 20.0                                              # every cuboid at one depth
        elif style < 0.4:
            par[:, :, 0] *= 0.05                                             # a narrow scene: everything reaches everything in x
        if rng.uniform() < 0.3 and N >= 8:
            bad = rng.integers(0, N, size=(B, 4))
            for b in range(B):
                par[b, bad[b, 0], 3] = 0.0                                    # zero width
                par[b, bad[b, 1], 5] = -1.0                                   # negative length
                par[b, bad[b, 2], 0] = np.nan
                par[b, bad[b, 3], 4] = np.inf
        thr = float(rng.choice([0.005, 0.2, 0.4, 0.55, 0.75]))
        counts = [N] + [int(rng.integers(1, N + 1)) for _ in range(B - 1)]
        ct = torch.tensor(counts, dtype=torch.int32).cuda()
        pt, st = torch.from_numpy(par).cuda(), torch.from_numpy(scores).cuda()
        one = G.differentiable_nms_with_iou3d_batched(st, pt, counts=ct, nms_threshold=thr)
        two = G.differentiable_nms_batched(st, one[6], counts=ct, nms_threshold=thr)
        tag = (trial, B, N, clustered, thr, counts)
        for b in range(B):
            n = counts[b]
            m = one[6][b, :n, :n]
            if not torch.isfinite(m).all():
                continue                                                      # NaN overlaps: the order among NaN rows is the sort's, compared elsewhere
            assert torch.equal(one[0][b, :n], two[0][b, :n]), tag
            assert int(one[4][b]) == int(two[4][b]) and torch.equal(one[2][b, :int(one[4][b])], two[2][b, :int(two[4][b])]), tag


@pytest.mark.gpu
def test_empty_images_and_the_fast_tail_on_poisoned_outputs(G, O):
    """an image with counts[b] == 0 must still get its outputs -- the symmetric scan's one (empty) super-block has to reach
    K6, the only writer of prob / nvalid / ninvalid / the index lists.  Every entry that takes that scan (one-call 2D / 3D, from boxes, matrix-in
    with the symmetry check from N = 256), output buffers POISONED before the call (0xff bytes: NaN probabilities, -1 counts would pass as
    padding, so the lists are poisoned with 0x7f) and compared over the FULL rows; counts that leave whole super-blocks of the launch without
    work; and the non-empty images of the same batch against the oracle, gradients included (the fast tail's CSR workgroup built the runs)."""
    import ctypes
    from groomed_nms_amd import synthetic, _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, check
    lib = _lib.load()
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    dev = torch.device("cuda")
    for dim, N, counts in ((2, 256, [0, 256, 0, 100]), (2, 1024, [0, 1024, 1, 0]), (2, 4096, [0, 4096, 1024, 1025, 0]), (2, 8192, [0, 8192, 100]),
                           (3, 256, [0, 256, 7]), (3, 2048, [2048, 0, 1000]), (3, 4096, [0, 3000, 0]), (2, 3000, [0, 0, 0])):
        B = len(counts)
        if dim == 2:
            src_np, sc_np = synthetic.batch_2d(50 + N, B, N, "uniform")
        else:
            src_np, sc_np = synthetic.batch_3d(50 + N, B, N, clustered=False)
        src, sc = torch.from_numpy(src_np).to(dev), torch.from_numpy(sc_np).to(dev)
        ct = torch.tensor(counts, dtype=torch.int32, device=dev)
        nbytes = lib.gnms_workspace_bytes(B, N, ctypes.byref(P))
        wgt = torch.linspace(-1.0, 2.0, N, device=dev).repeat(B, 1).contiguous()
        entries = ("one_call", "matrix_in") + (("from_boxes",) if dim == 2 else ())
        for entry in entries:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev).fill_(0xA5)
            iou = torch.empty((B, N, N), device=dev)
            prob = torch.empty((B, N), device=dev)
            prob.view(torch.uint8).fill_(0xFF)
            valid = torch.empty((B, N), dtype=torch.int64, device=dev)
            invalid = torch.empty((B, N), dtype=torch.int64, device=dev)
            valid.view(torch.uint8).fill_(0x7F)
            invalid.view(torch.uint8).fill_(0x7F)
            nv = torch.full((B,), -7, dtype=torch.int32, device=dev)
            ni = torch.full((B,), -7, dtype=torch.int32, device=dev)
            grad = torch.empty((B, N), device=dev)
            grad.view(torch.uint8).fill_(0xFF)
            if entry == "one_call":
                fwd = lib.gnms_forward_with_iou2d if dim == 2 else lib.gnms_forward_with_iou3d
                check(fwd(ptr(src), ptr(sc), B, N, N, ptr(ct), ctypes.byref(P), ptr(iou), ptr(prob), None, ptr(valid), ptr(invalid), ptr(nv), ptr(ni),
                          ptr(ws), nbytes, None), "fwd")
            elif entry == "from_boxes":
                check(lib.gnms_forward_from_boxes(ptr(src), ptr(sc), B, N, ptr(ct), ctypes.byref(P), ptr(prob), None, ptr(valid), ptr(invalid), ptr(nv),
                                                  ptr(ni), ptr(ws), nbytes, None), "fwd")
            else:
                if dim == 2:
                    check(lib.gnms_iou2d(ptr(src), ptr(src), B, N, N, ptr(iou), N, None), "iou2d")
                else:
                    check(lib.gnms_nms_overlap3d_from_params(ptr(src), B, N, float(P.nms_threshold), ptr(iou), N, None), "overlap3d")
                check(lib.gnms_forward(ptr(sc), ptr(iou), B, N, N, ptr(ct), ctypes.byref(P), ptr(prob), None, ptr(valid), ptr(invalid), ptr(nv), ptr(ni),
                                       ptr(ws), nbytes, None), "fwd")
            check(lib.gnms_backward(ptr(wgt), ptr(sc), ptr(iou), B, N, N, ptr(ct), ctypes.byref(P), ptr(grad), None, ptr(ws), nbytes, None), "bwd")
            torch.cuda.synchronize()
            for b in range(B):
                n, tag = counts[b], (dim, N, entry, b)
                k, j = int(nv[b]), int(ni[b])
                assert k >= 0 and j >= 0 and k + j <= n, tag
                pb = prob[b].cpu().numpy()
                assert np.all(pb[n:] == 0), tag                                     # (no NaN poison left: every entry of the row was written)
                assert torch.all(valid[b, k:] == -1) and torch.all(invalid[b, j:] == -1), tag
                assert torch.all(grad[b, n:] == 0), tag
                if n == 0:
                    continue
                if dim == 2:
                    m = O.iou2d(src_np[b, :n], src_np[b, :n])
                else:
                    m = _oracle_overlap3d(O, O.corners_of_cuboid(src_np[b, :n]))
                ref = O.differentiable_nms(sc_np[b, :n], m, grad_prob=wgt[b, :n].cpu().numpy())
                if dim == 2:
                    assert np.array_equal(pb[:n], ref["prob"]), tag
                    assert valid[b, :k].tolist() == list(ref["valid"]) and invalid[b, :j].tolist() == list(ref["invalid"]), tag
                    assert np.array_equal(grad[b, :n].cpu().numpy(), ref["grad_scores"]), tag
                else:                                                               # (guard band of the 3D overlap: TOL, conftest)
                    np.testing.assert_allclose(pb[:n], ref["prob"], atol=TOL, err_msg=str(tag))
                    np.testing.assert_allclose(grad[b, :n].cpu().numpy(), ref["grad_scores"], atol=TOL, rtol=1e-4, err_msg=str(tag))
                    check_index_lists(valid[b, :k].cpu().numpy(), invalid[b, :j].cpu().numpy(), ref["valid"], ref["invalid"])


@pytest.mark.gpu
def test_fuzz_3d_one_call_against_the_oracle(G, O):
    """the 3D one-call entry against the ORACLE (not against its own matrix): seeded cuboid sets -- clustered and uniform,
    flat and narrow scenes, ragged counts, thresholds around the cull's limit, box counts on both sides of 64 / 1024 / 2048 -- through
    records -> column sort -> slot-culled bit matrix -> scan / fast tail, compared with corners -> iou3d_approximate(generalized) ->
    0.5 (1 + giou) -> differentiable_nms of the CPU restatement: probabilities and gradients within TOL (the guard band of the 3D overlap,
    iou3d_pair.h), valid / invalid as sets; an image is skipped when an overlap sits within 2e-6 of the threshold (the two sides may then
    legitimately differ by a whole box: SURVEY 8-a6) -- counted, and it must stay the exception."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(20261001)
    checked = skipped = 0
    for trial in range(36):
        B = int(rng.integers(1, 4))
        N = int(rng.choice([5, 63, 64, 65, 257, 700, 1024, 1025, 1500, 2049, 2300]))
        clustered = bool(rng.uniform() < 0.5)
        par, scores = synthetic.batch_3d(int(rng.integers(1 << 30)), B, N, clustered=clustered, per=int(rng.choice([4, 32, 120])))
        style = rng.uniform()
        if style < 0.2:
            par[:, :, 2] = 20.0                                              # every cuboid at one depth
        elif style < 0.4:
            par[:, :, 0] *= 0.05                                             # a narrow scene
        thr = float(rng.choice([0.2, 0.4, 0.55, 0.75]))
        gs = int(rng.choice([100, 100, 3]))
        counts = [N] + [int(rng.integers(1, N + 1)) for _ in range(B - 1)]
        ct = torch.tensor(counts, dtype=torch.int32).cuda()
        pt = torch.from_numpy(par).cuda()
        st = torch.from_numpy(scores).cuda().requires_grad_(True)
        w = torch.from_numpy(rng.uniform(-1, 2, (B, N)).astype(np.float32)).cuda()
        out = G.differentiable_nms_with_iou3d_batched(st, pt, counts=ct, nms_threshold=thr, group_size=gs)
        (out[0] * w).sum().backward()
        tag = (trial, B, N, clustered, thr, gs, counts)
        for b in range(B):
            n = counts[b]
            m = _oracle_overlap3d(O, O.corners_of_cuboid(par[b, :n]))
            if np.any(np.abs(m - np.float32(thr)) < 2e-6):
                skipped += 1
                continue
            ref = O.differentiable_nms(scores[b, :n], m, grad_prob=w[b, :n].cpu().numpy(), nms_threshold=thr, group_size=gs)
            np.testing.assert_allclose(out[0][b, :n].detach().cpu().numpy(), ref["prob"], atol=TOL, err_msg=str(tag))
            np.testing.assert_allclose(st.grad[b, :n].cpu().numpy(), ref["grad_scores"], atol=TOL, rtol=1e-4, err_msg=str(tag))
            nv, ni = int(out[4][b]), int(out[5][b])
            check_index_lists(out[2][b, :nv].cpu().numpy(), out[3][b, :ni].cpu().numpy(), ref["valid"], ref["invalid"])
            np.testing.assert_allclose(out[6][b, :n, :n].cpu().numpy(), m, atol=TOL, err_msg=str(tag))
            checked += 1
    assert checked >= 40 and skipped <= checked // 4, (checked, skipped)


@pytest.mark.gpu
def test_indices_copy_on_device_tensors(golden_misc):
    """a9 (lib/groomed_nms.py:272-337) on the GPU box: the golden case and the layer's own use of it in the reference -- scattering a group's
    block into the N x N inversion matrix (:108) -- with every tensor on the device; results against the reference's golden output and
    against plain indexing."""
    from groomed_nms_amd import indices_copy
    g = golden_misc
    dev = torch.device("cuda")
    A = torch.from_numpy(g["indices_copy/A"].copy()).to(dev)
    out = indices_copy(A, torch.from_numpy(g["indices_copy/B"]).to(dev), torch.from_numpy(g["indices_copy/ind"]).to(dev))
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), g["indices_copy/out"])
    assert out.data_ptr() == A.data_ptr()                                          # in place, as the reference (:331-337)
    rng = np.random.default_rng(5)
    n = 300
    M = torch.zeros((n, n), device=dev)
    grp = torch.from_numpy(np.sort(rng.choice(n, 37, replace=False))).to(dev)
    blk = torch.from_numpy(rng.standard_normal((37, 37)).astype(np.float32)).to(dev)
    ref = M.clone()
    ref[grp[:, None], grp[None, :]] = blk
    got = indices_copy(M, blk, grp)
    assert torch.equal(got, ref)
    keep = M.clone()
    got2 = indices_copy(M, 2 * blk, grp, inplace=False)
    assert torch.equal(M, keep) and torch.equal(got2[grp[:, None], grp[None, :]], 2 * blk)


@pytest.mark.gpu
def test_inference_tail_nms_to_kitti_text(G, O):
    """f4 on the GPU box: the reference's inference tail, lib/rpn_util.py:1295-1319 + :1385-1487 -- float64 proposals ->
    iou(aboxes, aboxes) (NumPy in: the float64 HIP kernel) -> differentiable_nms on NumPy inputs -> `[0].numpy()` keep list -> the kept rows
    through kitti_io -- on the golden KITTI cases: the keep list equals the oracle's on the same float64 overlaps, and every line written for
    a kept box is, byte for byte, the line the REFERENCE wrote for that box (tests/golden/kitti_io.npz holds its text for all boxes)."""
    from conftest import Golden
    from groomed_nms_amd import kitti_io as K, overlaps
    g = Golden("kitti_io.npz")

    class Conf(dict):
        __getattr__ = dict.__getitem__
    for tag in ("k12", "k40_un"):
        conf = Conf(lbls=["Car", "Pedestrian", "Cyclist"], has_un=bool(g[f"{tag}/has_un"]), use_un_for_score=bool(g[f"{tag}/has_un"]))
        aboxes = g[f"{tag}/boxes"]                                                 # float64 [n, 14]: x1 y1 x2 y2 score cls ...
        m = overlaps.iou(aboxes[:, 0:4], aboxes[:, 0:4])                           # lib/rpn_util.py:1295-1300 (NumPy float64 in and out)
        assert isinstance(m, np.ndarray) and m.dtype == np.float64
        keep = G.differentiable_nms(aboxes[:, 4], m, nms_threshold=0.4)[0].numpy()  # :1319-1320
        ref = O.differentiable_nms(aboxes[:, 4].astype(np.float32), O.iou2d_f64(aboxes[:, 0:4], aboxes[:, 0:4]).astype(np.float32), nms_threshold=0.4)
        assert keep.tolist() == [int(i) for i in ref["valid"]], tag
        assert 0 < len(keep) < len(aboxes), tag                                    # (the case suppresses something and keeps something)
        kept = aboxes[keep]
        conv = K.convert_image_predictions_to_correct_entries(kept, conf, g[f"{tag}/p2"])
        text = K.get_text_to_write_in_kitti_format(conv, conf)
        golden_lines = g[f"{tag}/text"].tobytes().decode().split("\n")
        lines = text.split("\n")
        assert lines[-1] == "" and len(lines) - 1 == len(keep), tag
        for line, i in zip(lines[:-1], keep.tolist()):
            assert line == golden_lines[i], (tag, i)


@pytest.mark.gpu
def test_training_tail_in_one_host_call(G):
    """Round 5 (VERDICT r4 #4a): the layer's neighbours on the C++ host path and the training tail of lib/loss/rpn_3d.py:772-825 + :1117-1131
    as ONE call (proposals.training_tail: layer -> best box per ground truth -> after-NMS AP loss).  Against the same chain made of the
    separate entries (each of which is held to the oracle / the reference's vectors by its own test): loss, probabilities, targets and
    dL/dscores bit for bit; ragged counts; and captured into a HIP graph and replayed on new inputs (nothing but stream-ordered launches)."""
    from groomed_nms_amd import proposals as PR, synthetic
    from groomed_nms_amd.aploss import ap_loss_batched
    rng = np.random.default_rng(99)
    B, N, M = 3, 700, 6
    dev = torch.device("cuda")

    def draw(seed):
        b2, sc = synthetic.batch_2d(seed, B, N, "clustered", per=24)
        p3, _ = synthetic.batch_3d(seed + 1, B, N, clustered=True, per=24)
        o = np.argsort(-sc, axis=1, kind="stable")                                 # the loss sorts by score first (:731-737)
        sc, b2, p3 = np.take_along_axis(sc, o, 1), np.take_along_axis(b2, o[:, :, None], 1), np.take_along_axis(p3, o[:, :, None], 1)
        pick = np.stack([np.random.default_rng(seed + b).choice(N // 2, M, replace=False) for b in range(B)])
        return sc, b2, p3, np.take_along_axis(p3, pick[:, :, None], 1).copy(), np.take_along_axis(b2, pick[:, :, None], 1).copy()
    counts = torch.tensor([N, 431, 64], dtype=torch.int32, device=dev)
    gtc = torch.tensor([M, 3, 1], dtype=torch.int32, device=dev)
    sc, b2, p3, gp, gb = draw(5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s1, s2 = t(sc).requires_grad_(True), t(sc).requires_grad_(True)
    loss, prob, targets = PR.training_tail(s1, t(b2), t(p3), t(gp), t(gb), 0.3, counts=counts, gt_counts=gtc)
    prob2 = G.differentiable_nms_with_iou2d_batched(s2, t(b2), counts=counts, index_lists=False)[0]
    targets2 = PR.best_targets(t(p3), t(b2), t(gp), t(gb), 0.3, pred_counts=counts, gt_counts=gtc)[0]
    loss2 = ap_loss_batched(prob2, targets2, counts=counts)
    assert torch.equal(prob, prob2) and torch.equal(targets, targets2) and torch.equal(loss, loss2)
    assert float(targets.sum()) >= 3 and torch.all(loss >= 0)
    wl = torch.tensor([1.0, 0.5, 2.0], device=dev)
    (loss * wl).sum().backward()
    (loss2 * wl).sum().backward()
    assert torch.equal(s1.grad, s2.grad) and float(s1.grad.abs().sum()) > 0
    # captured and replayed on new inputs
    bufs = [torch.empty_like(t(x)) for x in (sc, b2, p3, gp, gb)]
    for dst, src in zip(bufs, (sc, b2, p3, gp, gb)):
        dst.copy_(t(src))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            PR.training_tail(*bufs, 0.3, counts=counts, gt_counts=gtc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss, g_prob, g_tg = PR.training_tail(*bufs, 0.3, counts=counts, gt_counts=gtc)
    for seed in (6, 7):
        new = draw(seed)
        for dst, src in zip(bufs, new):
            dst.copy_(t(src))
        graph.replay()
        e_loss, e_prob, e_tg = PR.training_tail(*[t(x) for x in new], 0.3, counts=counts, gt_counts=gtc)
        assert torch.equal(g_loss, e_loss) and torch.equal(g_prob, e_prob) and torch.equal(g_tg, e_tg), seed


@pytest.mark.gpu
def test_fast_tail_corner_cases_against_oracle(G, O):
    """The fast tail's fallbacks (round 5), each against the oracle, bit for bit, with gradients:
    * scores that nearly TIE (what a randomly initialised RPN emits -- the C3 harness: 4096 scores within 3e-3 of 0.76): every rescored
      member lands behind the last head, i.e. in ONE bucket of K6's merge -> B goes through the sort;
    * a cap far above the group lengths with one dense cluster of more than 256 boxes -> K5 proper (the CSR workgroup would rank the
      run's members by comparison);
    * a few heads and many valid members; no valid box at all; every box valid."""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(31)
    cases = []
    bx, _ = synthetic.batch_2d(1, 1, 4096, "clustered", per=3)
    cases.append(("near ties", bx[0], (0.76 - 1e-7 * rng.permutation(4096)).astype(np.float32), {}))
    bx, sc = synthetic.batch_2d(2, 1, 3000, "clustered", per=600)
    cases.append(("long groups", bx[0], sc[0], dict(group_size=5000)))
    bx, sc = synthetic.batch_2d(3, 1, 2500, "clustered", per=90)
    cases.append(("few heads", bx[0], (0.9 + 0.1 * sc[0]).astype(np.float32), dict(valid_box_prob_threshold=0.2)))
    bx, sc = synthetic.batch_2d(4, 1, 1500, "uniform")
    cases.append(("none valid", bx[0], (0.2 * sc[0]).astype(np.float32), {}))
    cases.append(("all valid", bx[0], (0.5 + 0.5 * sc[0]).astype(np.float32), dict(valid_box_prob_threshold=0.0)))
    for tag, boxes, scores, kw in cases:
        n = len(scores)
        st = torch.from_numpy(scores[None]).cuda().requires_grad_(True)
        w = torch.from_numpy(rng.uniform(-1, 2, (1, n)).astype(np.float32)).cuda()
        out = G.differentiable_nms_with_iou2d_batched(st, torch.from_numpy(boxes[None]).cuda(), **kw)
        (out[0] * w).sum().backward()
        ref = O.differentiable_nms(scores, O.iou2d(boxes, boxes), grad_prob=w[0].cpu().numpy(), **kw)
        assert np.array_equal(out[0][0].detach().cpu().numpy(), ref["prob"]), tag
        nv, ni = int(out[4][0]), int(out[5][0])
        assert out[2][0, :nv].tolist() == list(ref["valid"]) and out[3][0, :ni].tolist() == list(ref["invalid"]), tag
        assert np.array_equal(st.grad[0].cpu().numpy(), ref["grad_scores"]), tag


@pytest.mark.gpu
def test_counts_to_host_mailbox(G):
    """gnms_counts_to_host (the host round trip of lib/groomed_nms.py:120-127 as a tag-polled slot of pinned memory): the counts it hands
    to the host equal a plain device-to-host copy -- every B up to the slot size, the copy path above it, both bindings, calls right behind
    a long-running kernel (the tag must not be seen early), four host threads with streams of their own at once, and a refusal inside a
    stream capture; differentiable_nms's index tensors go through it on every call (lengths against nvalid of the batched entry)."""
    import ctypes
    import threading
    from groomed_nms_amd import _lib, groomed_nms as M, synthetic
    from groomed_nms_amd.overlaps import iou as iou_fn
    lib = _lib.load()
    dev = torch.device("cuda")
    rng = np.random.default_rng(77)
    ext = M._binding()
    assert ext and hasattr(ext, "counts_to_host")

    def via_ctypes(nv, ni):
        b = nv.shape[0]
        host = (ctypes.c_int32 * (2 * b))()
        _lib.check(lib.gnms_counts_to_host(nv.data_ptr(), ni.data_ptr(), b, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)), "counts")
        return list(host)

    for B in (1, 2, 8, 63, 64, 65, 127, 128, 300):          # 127 = the last B of the mailbox, from 128 on the copy path
        for rep in range(3):
            a = rng.integers(0, 1 << 30, B).astype(np.int32)
            b = rng.integers(0, 1 << 30, B).astype(np.int32)
            nv, ni = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            want = a.tolist() + b.tolist()
            assert list(ext.counts_to_host(nv, ni)) == want, (B, rep)
            assert via_ctypes(nv, ni) == want, (B, rep)
            assert M._counts_to_host(nv, ni) == want
    # behind ~2 ms of queued work that produces the counts: the poll must wait for the producer
    big = torch.zeros((1 << 24,), dtype=torch.int32, device=dev)
    for rep in range(20):
        big.add_(1)
        big.add_(1)
        nv = big[:4].clone()
        ni = big[-4:].clone()
        assert list(ext.counts_to_host(nv, ni)) == [2 * (rep + 1)] * 8
    # more calls than slots (the slot of a tag is reused every 64 calls)
    for rep in range(200):
        nv = torch.full((3,), rep, dtype=torch.int32, device=dev)
        assert list(ext.counts_to_host(nv, nv)) == [rep] * 6
    # four host threads, a stream each
    errs = []

    def worker(t):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(150):
                    nv = torch.full((5,), 1000 * t + rep, dtype=torch.int32, device=dev)
                    ni = nv + 7
                    got = list(ext.counts_to_host(nv, ni))
                    if got != [1000 * t + rep] * 5 + [1000 * t + rep + 7] * 5:
                        errs.append((t, rep, got))
        except Exception as e:                                # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs[:3]
    # no host round trip inside a capture
    nv = torch.zeros((2,), dtype=torch.int32, device=dev)
    cap_b, cap_sc = synthetic.batch_2d(3, 1, 300, "uniform")
    cap_s = torch.from_numpy(cap_sc[0]).to(dev)
    cap_iou = iou_fn(torch.from_numpy(cap_b[0]).to(dev), torch.from_numpy(cap_b[0]).to(dev))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g.capture_begin()
        try:
            with pytest.raises(_lib.GnmsError):
                via_ctypes(nv, nv)
            with pytest.raises(RuntimeError, match="cannot be captured"):          # the reference entry says so before it launches anything
                G.differentiable_nms(cap_s, cap_iou)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    # the slot form (gnms_host_counts_slot / _wait): the forward call's own stores land in pinned memory
    P = _lib.GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    for B, n in ((1, 500), (3, 300), (8, 1024)):
        boxes, scores = synthetic.batch_2d(900 + n, B, n, "uniform")
        bt, sc = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
        ref = G.differentiable_nms_with_iou2d_batched(sc, bt)
        dv, hv = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.gnms_host_counts_slot(B, ctypes.byref(dv), ctypes.byref(hv)), "slot")
        preset = (ctypes.c_int32 * (2 * B)).from_address(hv.value)
        assert list(preset) == [-1] * (2 * B)
        ws = torch.empty((lib.gnms_workspace_bytes(B, n, ctypes.byref(P)),), dtype=torch.uint8, device=dev)
        prob = torch.empty((B, n), device=dev)
        iou = torch.empty((B, n, n), device=dev)
        _lib.check(lib.gnms_forward_with_iou2d(bt.data_ptr(), sc.data_ptr(), B, n, n, None, ctypes.byref(P), iou.data_ptr(), prob.data_ptr(), None, None, None,
                                               dv.value, dv.value + 4 * B, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "fwd")
        host = (ctypes.c_int32 * (2 * B))()
        _lib.check(lib.gnms_host_counts_wait(hv.value, B, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)), "wait")
        assert list(host) == ref[4].tolist() + ref[5].tolist(), (B, n)
        assert torch.equal(prob, ref[0])
    dv, hv = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.gnms_host_counts_slot(2, ctypes.byref(dv), ctypes.byref(hv)), "slot")
    host = (ctypes.c_int32 * 4)()
    torch.cuda.synchronize()
    assert lib.gnms_host_counts_wait(hv.value, 2, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)) == -1        # nobody writes this slot
    assert b"never written" in lib.gnms_last_error()
    assert lib.gnms_host_counts_slot(128, ctypes.byref(dv), ctypes.byref(hv)) == -2
    # the reference entry: lengths of the two index tensors = the batched entry's device-side counts
    for n in (1, 37, 500, 1500):
        boxes, scores = synthetic.batch_2d(300 + n, 1, n, "clustered")
        bt, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
        iou = iou_fn(bt[0], bt[0])
        valid, invalid, prob = G.differentiable_nms(s[0], iou)
        out = G.differentiable_nms_batched(s, iou.unsqueeze(0))
        assert valid.shape[0] == int(out[4][0]) and invalid.shape[0] == int(out[5][0]) and valid.shape[0] + invalid.shape[0] == n
        assert torch.equal(valid, out[2][0, :valid.shape[0]]) and torch.equal(invalid, out[3][0, :invalid.shape[0]])
        M.LAZY_INDEX_LISTS = True
        try:
            lv, li, lp = G.differentiable_nms(s[0], iou)
            assert isinstance(lv, M.LazyIndexList) and torch.equal(lv.t, valid) and torch.equal(li.t, invalid) and torch.equal(lp, prob)
        finally:
            M.LAZY_INDEX_LISTS = False


@pytest.mark.gpu
def test_counts_slot_ownership_under_threads(G):
    """VERDICT r5 #5 / ADVICE r5: a slot of the counts mailbox has ONE owner from gnms_host_counts_slot until its wait / release.  Eight host
    threads (a stream each) make 500 differentiable_nms(scores, iou) calls of different N at once -- far more than 64 slot hand-outs while
    any one thread sits between its slot and its wait; every call's index tensors must have the lengths AND contents of the batched
    entry's padded lists.  Then the same with the mailbox cut to two slots (gnms_test_mailbox_slots): most calls find no free slot and take
    the plain path, none may read another call's counts.  Then the protocol itself through the C ABI: a leaked slot is never handed out
    again, release gives it back, a second wait on a view is refused."""
    import ctypes
    import threading
    from groomed_nms_amd import _lib, groomed_nms as M, synthetic
    from groomed_nms_amd.overlaps import iou as iou_fn
    lib = _lib.load()
    dev = torch.device("cuda")
    ext = M._binding()
    assert ext and hasattr(ext, "single")
    sizes = [3, 17, 64, 100, 129, 257, 300, 411, 500, 640, 777, 1024]
    cases = []
    for i, n in enumerate(sizes):
        boxes, scores = synthetic.batch_2d(4000 + i, 1, n, "clustered" if i % 2 else "uniform")
        bt, s = torch.from_numpy(boxes[0]).to(dev), torch.from_numpy(scores[0]).to(dev)
        iou = iou_fn(bt, bt)
        ref = G.differentiable_nms_batched(s.unsqueeze(0), iou.unsqueeze(0))
        k, m = int(ref[4][0]), int(ref[5][0])
        cases.append((s, iou, ref[2][0, :k].clone(), ref[3][0, :m].clone(), ref[0][0].clone()))
    torch.cuda.synchronize()
    assert len({c[2].shape[0] for c in cases}) >= 8           # the lengths differ from case to case: a stolen slot would show

    def storm(threads, calls):
        errs = []

        def worker(t):
            try:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    for rep in range(calls):
                        s, iou, v, iv, pr = cases[(7 * t + rep) % len(cases)]
                        valid, invalid, prob = G.differentiable_nms(s, iou)
                        if valid.shape != v.shape or invalid.shape != iv.shape:
                            errs.append((t, rep, "length", tuple(valid.shape), tuple(v.shape)))
                        elif rep % 8 == 0 and not (torch.equal(valid, v) and torch.equal(invalid, iv) and torch.equal(prob, pr)):
                            errs.append((t, rep, "content"))
            except Exception as e:                            # noqa: BLE001
                errs.append((t, repr(e)))
        th = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
        [x.start() for x in th]
        [x.join() for x in th]
        return errs

    assert M.LAZY_INDEX_LISTS is False
    errs = storm(8, 500)
    assert not errs, errs[:4]
    old = lib.gnms_test_mailbox_slots(2)
    try:
        errs = storm(8, 500)
        assert not errs, errs[:4]
        # the protocol: two slots, both taken -> the third request is refused, not served with an owned slot
        dv, hv = [ctypes.c_void_p() for _ in range(3)], [ctypes.c_void_p() for _ in range(3)]
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[0]), ctypes.byref(hv[0])) == 0
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[1]), ctypes.byref(hv[1])) == 0
        assert hv[0].value != hv[1].value
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[2]), ctypes.byref(hv[2])) == -2 and b"owned" in lib.gnms_last_error()
        # ... and the tagged path falls back to its copy while every slot is owned
        nv = torch.tensor([41, 42], dtype=torch.int32, device=dev)
        assert list(ext.counts_to_host(nv, nv + 1)) == [41, 42, 42, 43]
        # a forward call into slot 0; its wait gives the slot back; a second wait on the same view is refused
        s, iou, v, iv, pr = cases[8]
        n = s.shape[0]
        P = _lib.GnmsParams()
        lib.gnms_default_params(ctypes.byref(P))
        ws = torch.empty((lib.gnms_workspace_bytes(1, n, ctypes.byref(P)),), dtype=torch.uint8, device=dev)
        prob = torch.empty((1, n), device=dev)
        _lib.check(lib.gnms_forward(s.data_ptr(), iou.data_ptr(), 1, n, n, None, ctypes.byref(P), prob.data_ptr(), None, None, None,
                                    dv[0].value, dv[0].value + 4, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "fwd")
        host = (ctypes.c_int32 * 2)()
        _lib.check(lib.gnms_host_counts_wait(hv[0].value, 1, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)), "wait")
        assert list(host) == [v.shape[0], iv.shape[0]]
        assert lib.gnms_host_counts_wait(hv[0].value, 1, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)) == -1 and b"not owned" in lib.gnms_last_error()
        assert lib.gnms_host_counts_wait(hv[0].value + 4, 1, ctypes.cast(host, ctypes.c_void_p), _lib.stream_ptr(dev)) == -1     # not a view
        # slot 0 is free again, slot 1 still owned; release returns it
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[2]), ctypes.byref(hv[2])) == 0 and hv[2].value == hv[0].value
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[0]), ctypes.byref(hv[0])) == -2
        _lib.check(lib.gnms_host_counts_release(hv[1].value, _lib.stream_ptr(dev)), "release")
        assert lib.gnms_host_counts_release(hv[1].value, _lib.stream_ptr(dev)) == -1
        _lib.check(lib.gnms_host_counts_release(hv[2].value, _lib.stream_ptr(dev)), "release")
        # a forward call that raises inside differentiable_nms (refused parameters) must not leak its slot: with two slots, three failures
        # in a row would leave none
        bb, bs = synthetic.batch_2d(4100, 1, 2100, "uniform")          # N above the largest unmasked group the solves take: gnms_forward refuses
        bbt = torch.from_numpy(bb[0]).to(dev)
        big_s, big_iou = torch.from_numpy(bs[0]).to(dev), iou_fn(bbt, bbt)
        for _ in range(3):
            with pytest.raises(_lib.GnmsError, match="unmasked groups"):
                G.differentiable_nms(big_s, big_iou, mask_group_boxes=False, group_size=1 << 20)
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[0]), ctypes.byref(hv[0])) == 0
        assert lib.gnms_host_counts_slot(1, ctypes.byref(dv[1]), ctypes.byref(hv[1])) == 0
        _lib.check(lib.gnms_host_counts_release(hv[0].value, _lib.stream_ptr(dev)), "release")
        _lib.check(lib.gnms_host_counts_release(hv[1].value, _lib.stream_ptr(dev)), "release")
    finally:
        lib.gnms_test_mailbox_slots(old)
    valid, invalid, prob = G.differentiable_nms(cases[8][0], cases[8][1])
    assert torch.equal(valid, cases[8][2]) and torch.equal(invalid, cases[8][3])


@pytest.mark.gpu
def test_one_launch_against_three_launches(O):
    """Round 6: up to N = 1024 the matrix-in layer is ONE launch (one_launch_kernel: sort, the scan's table straight from the matrix, chain;
    nms_one_launch.h); GNMS_ONE_LAUNCH=0 keeps the three launches (sort_count_kernel, bitmask_small_kernel, tail_kernel with the symmetry check).
    The one-call entry's launch builds its table in rank space up to one round of tasks and with the sources in x order beyond (B = 8, N = 1024;
    ragged B = 16, N = 512; B = 4, N = 768; pixel-grid boxes).
    Probabilities, order, lists, counts and gradients of the two are the same bit for bit -- sizes around the 64-row and 256-column edges,
    batches (ragged, with an empty image), already sorted scores, the presorted mode (never the one launch), an asymmetric matrix (the one
    launch reads the reference's own triangle, the three launches find the asymmetry and take the general scan), NaN entries (:250 removes
    them), a strided matrix view (ld > N), an odd ld (never the one launch), groups above the cap (verdict "slow": K5 proper inside the launch),
    negative thresholds, the same call repeated, single images through the reference's own signature -- and the default run equals the oracle
    (the launch inside a captured graph: test_capturable_in_a_hip_graph, N = 1024)."""
    code = """
import sys, numpy as np, torch
import groomed_nms_amd as G
from groomed_nms_amd import synthetic, overlaps
out = {}
def run(tag, s, m, counts=None, **kw):
    st = s.clone().requires_grad_(True)
    o = G.differentiable_nms_batched(st, m, counts=counts, **kw)
    w = torch.linspace(-1.0, 2.0, s.shape[1], device="cuda").repeat(s.shape[0], 1)
    (o[0] * w).sum().backward()
    for i, k in enumerate(("prob", "order", "valid", "invalid", "nvalid", "ninvalid")):
        a = o[i].detach().cpu().numpy().copy()
        if k in ("valid", "invalid"):                       # padded behind the counts
            cnt = o[4 if k == "valid" else 5].cpu().numpy()
            for b in range(a.shape[0]):
                a[b, cnt[b]:] = -1
        out[tag + "_" + k] = a
    g = st.grad.cpu().numpy().copy()
    if counts is not None:
        c = counts.cpu().numpy()
        for b in range(g.shape[0]):
            g[b, c[b]:] = 0
            out[tag + "_prob"][b, c[b]:] = 0
            out[tag + "_order"][b, c[b]:] = -1
    out[tag + "_grad"] = g
for n in (1, 2, 63, 64, 65, 200, 255, 256, 257, 500, 511, 513, 777, 1000, 1024, 1500, 2048):
    for kind in ("uniform", "clustered"):
        b, s = synthetic.batch_2d(40 + n, 1, n, kind)
        bt, st = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
        run("n%d_%s" % (n, kind), st, overlaps.iou_batched(bt))
b, s = synthetic.batch_2d(5, 5, 700, "clustered")
bt, st = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
m = overlaps.iou_batched(bt)
run("ragged", st, m, counts=torch.tensor([700, 0, 1, 333, 65], dtype=torch.int32, device="cuda"))
o = torch.sort(st, dim=1, descending=True, stable=True)[1]
ss = torch.gather(st, 1, o)
ms = torch.gather(torch.gather(m, 1, o[:, :, None].expand(-1, -1, 700)), 2, o[:, None, :].expand(-1, 700, -1)).contiguous()
run("sorted", ss, ms)
run("presorted", ss, ms, presorted=True)
ma = m.clone(); ma[:, 3, 40:90] = 0.9; ma[:, 400:420, 7] = 0.0
run("asym", st, ma)
mn = m.clone(); mn[:, 10, 20] = float("nan"); mn[:, 20, 10] = float("nan"); mn[:, 5, 600] = float("nan")
run("nan", st, mn)
wide = torch.zeros((5, 700, 704), device="cuda"); wide[:, :, :700] = m
run("strided", st, wide[:, :, :700])
odd = torch.zeros((5, 700, 701), device="cuda"); odd[:, :, :700] = m
run("odd_ld", st, odd[:, :, :700])                      # (ld % 4 != 0: the scalar row kernel either way)
b8, s8 = synthetic.batch_2d(9, 8, 1024, "uniform")
m8 = overlaps.iou_batched(torch.from_numpy(b8).cuda())
run("b8_n1024", torch.from_numpy(s8).cuda(), m8)
b3, s3 = synthetic.batch_2d(10, 3, 500, "clustered", per=25)
m3 = overlaps.iou_batched(torch.from_numpy(b3).cuda())
for gs in (2, 30, 100):
    run("cap%d" % gs, torch.from_numpy(s3).cuda(), m3, group_size=gs)
run("negthr", torch.from_numpy(s3).cuda(), m3, nms_threshold=-0.5)
run("thr0", torch.from_numpy(s3).cuda(), m3, nms_threshold=0.0)
run("sorted_prob", torch.from_numpy(s3).cuda(), m3, return_sorted_prob=True)
for rep in range(3):                                     # the call counter moves on, stale flags never match
    run("rep%d" % rep, torch.from_numpy(s3).cuda(), m3)
# the one-call entry (boxes in, matrix + layer out): one_launch_boxes_kernel against sort + bits + tail_write_kernel
def run_boxes(tag, bx, sc, counts=None, **kw):
    st = sc.clone().requires_grad_(True)
    o = G.differentiable_nms_with_iou2d_batched(st, bx, counts=counts, **kw)
    w = torch.linspace(-1.0, 2.0, sc.shape[1], device="cuda").repeat(sc.shape[0], 1)
    (o[0] * w).sum().backward()
    out[tag + "_w"] = w.cpu().numpy()
    c = counts.cpu().numpy() if counts is not None else None
    for i, k in enumerate(("prob", "order", "valid", "invalid", "nvalid", "ninvalid", "iou")):
        a = o[i].detach().cpu().numpy().copy()
        if k in ("valid", "invalid"):
            cnt = o[4 if k == "valid" else 5].cpu().numpy()
            for b in range(a.shape[0]):
                a[b, cnt[b]:] = -1
        if c is not None and k in ("prob", "order", "iou"):
            for b in range(a.shape[0]):
                if k == "iou":
                    a[b, c[b]:, :] = 0; a[b, :, c[b]:] = 0
                else:
                    a[b, c[b]:] = 0 if k == "prob" else -1
        out[tag + "_" + k] = a
    g = st.grad.cpu().numpy().copy()
    if c is not None:
        for b in range(g.shape[0]):
            g[b, c[b]:] = 0
    out[tag + "_grad"] = g
for n in (1, 2, 63, 64, 65, 200, 256, 257, 500, 777, 1000, 1024):
    for kind in ("uniform", "clustered"):
        b, s = synthetic.batch_2d(140 + n, 2, n, kind)
        run_boxes("box_n%d_%s" % (n, kind), torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda())
b, s = synthetic.batch_2d(15, 8, 1024, "uniform")
run_boxes("box_b8_n1024", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda())
b, s = synthetic.batch_2d(16, 8, 256, "clustered")
run_boxes("box_b8_n256", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda())
# (more than a round of rank-space table tasks: the table with its sources in x order, one_launch_bits_from_boxes_x)
b, s = synthetic.batch_2d(18, 16, 512, "clustered", per=30)
run_boxes("box_b16_n512", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(),
          counts=torch.tensor([512, 511, 65, 64, 63, 1, 0, 500, 512, 300, 129, 128, 127, 2, 448, 449], dtype=torch.int32, device="cuda"))
b, s = synthetic.batch_2d(19, 4, 768, "uniform")
run_boxes("box_b4_n768", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), nms_threshold=0.25)
b, s = synthetic.batch_2d(20, 3, 1000, "clustered", per=6)
run_boxes("box_b3_n1000_pixel", torch.from_numpy(np.round(b / 8) * 8).cuda(), torch.from_numpy(s).cuda())      # pixel-grid boxes: overlaps AT the threshold's neighbours, exact ties
b, s = synthetic.batch_2d(17, 5, 700, "clustered")
run_boxes("box_ragged", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), counts=torch.tensor([700, 0, 1, 333, 65], dtype=torch.int32, device="cuda"))
for gs in (2, 30):
    run_boxes("box_cap%d" % gs, torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), group_size=gs)
bd = b.copy(); bd[:, 5] = bd[:, 4]; bd[:, 9, 2] = bd[:, 9, 0]; bd[:, 11, 3] = np.float32("nan"); bd[:, 13] = np.float32(0.0)   # duplicates, an empty box, a NaN coordinate, an all-zero box
run_boxes("box_degenerate", torch.from_numpy(bd).cuda(), torch.from_numpy(s).cuda())
run_boxes("box_thr0", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), nms_threshold=0.0)
run_boxes("box_negthr", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), nms_threshold=-0.5)      # every pair set: a dense table, no cull
run_boxes("box_thr1", torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), nms_threshold=1.0)         # nothing but NaN overlaps set
for rep in range(3):
    run_boxes("box_rep%d" % rep, torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda())
# one image through the reference's own signature (index tensors through the pinned counts slot), twenty calls of alternating sizes
for i in range(20):
    n = (500, 130, 64, 1000)[i % 4]
    bb, ss = synthetic.batch_2d(60 + i, 1, n, "clustered", per=20)
    o = G.differentiable_nms(torch.from_numpy(ss[0]).cuda(), overlaps.iou(torch.from_numpy(bb[0]).cuda(), torch.from_numpy(bb[0]).cuda()))
    out["single%d_prob" % i], out["single%d_valid" % i], out["single%d_invalid" % i] = o[2].cpu().numpy(), o[0].cpu().numpy(), o[1].cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print("ok")
"""
    runs = {}
    for tag, env in (("default", {}), ("row_kernel", {"GNMS_ONE_LAUNCH": "0"})):
        path = "/tmp/gnms_one_launch_%s.npz" % tag
        r = _run_py(code, env, argv=(path,))
        assert r.returncode == 0 and "ok" in r.stdout, (tag, r.stderr[-2000:])
        runs[tag] = np.load(path)
    for k in runs["default"].files:
        assert np.array_equal(runs["row_kernel"][k], runs["default"][k], equal_nan=True), k
    # and the default run against the oracle on a few of the cases
    from groomed_nms_amd import synthetic
    d = runs["default"]
    for n, kind in ((65, "uniform"), (500, "clustered"), (1024, "uniform")):
        b, s = synthetic.batch_2d(140 + n, 2, n, kind)
        tag = "box_n%d_%s" % (n, kind)
        for img in range(2):
            m = O.iou2d(b[img], b[img])
            ref = O.differentiable_nms(s[img], m, grad_prob=d[tag + "_w"][img])
            np.testing.assert_array_equal(d[tag + "_iou"][img], m)
            np.testing.assert_array_equal(d[tag + "_prob"][img], ref["prob"])
            np.testing.assert_array_equal(d[tag + "_valid"][img, :int(d[tag + "_nvalid"][img])], ref["valid"])
            np.testing.assert_array_equal(d[tag + "_grad"][img], ref["grad_scores"])
    for n, kind in ((65, "clustered"), (500, "uniform"), (777, "clustered"), (1024, "uniform")):
        b, s = synthetic.batch_2d(40 + n, 1, n, kind)
        m = O.iou2d(b[0], b[0])
        ref = O.differentiable_nms(s[0], m)
        tag = "n%d_%s" % (n, kind)
        np.testing.assert_array_equal(d[tag + "_prob"][0], ref["prob"])
        nv = int(d[tag + "_nvalid"][0])
        np.testing.assert_array_equal(d[tag + "_valid"][0, :nv], ref["valid"])


@pytest.mark.gpu
def test_classic_nms_pinned_staging(O):
    """`_nms` keeps one block of pinned memory per device for the boxes, keep[] and the count (classic_nms.hip): a block that starts small
    (64 KiB) and has to grow between calls, sizes on both sides of the bit-matrix kernel's tile switch (64 x 64 tiles in a
    1D grid / 64 x 256 in a 2D grid), two host threads calling at once -- every keep list against the oracle."""
    code = """
import sys, threading, numpy as np
from groomed_nms_amd import synthetic
from groomed_nms_amd.nms import gpu_nms
out = {}
def dets_of(n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([synthetic.clustered_boxes_2d(rng, n, 32), synthetic.tie_free_scores(rng, n)[:, None]], 1).astype(np.float32)
for i, n in enumerate((500, 4096, 37, 9000, 500, 12000, 1)):
    out["seq%d_n%d" % (i, n)] = np.asarray(gpu_nms(dets_of(n, 10 + i), 0.45), np.int64)
res = {}
def worker(t):
    for rep in range(20):
        n = (300, 777, 2000, 64)[(t + rep) % 4]
        res[(t, rep)] = np.asarray(gpu_nms(dets_of(n, 1000 * t + rep), 0.5), np.int64)
th = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
[x.start() for x in th]; [x.join() for x in th]
for (t, rep), v in res.items():
    out["thr%d_%d" % (t, rep)] = v
np.savez(sys.argv[1], **out)
print("ok")
"""
    path = "/tmp/gnms_nms_stage.npz"
    r = _run_py(code, {}, argv=(path,))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    d = np.load(path)
    from groomed_nms_amd import synthetic

    def dets_of(n, seed):
        rng = np.random.default_rng(seed)
        return np.concatenate([synthetic.clustered_boxes_2d(rng, n, 32), synthetic.tie_free_scores(rng, n)[:, None]], 1).astype(np.float32)
    for i, n in enumerate((500, 4096, 37, 9000, 500, 12000, 1)):
        assert list(d["seq%d_n%d" % (i, n)]) == O.classic_nms(dets_of(n, 10 + i), 0.45, rule="gpu"), (i, n)
    for t in range(3):
        for rep in range(20):
            n = (300, 777, 2000, 64)[(t + rep) % 4]
            assert list(d["thr%d_%d" % (t, rep)]) == O.classic_nms(dets_of(n, 1000 * t + rep), 0.5, rule="gpu"), (t, rep)
