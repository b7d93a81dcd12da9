"""dL/d(overlap matrix) of the layer against the CPU oracle behind every forward route and on every backward route.

The matrix gradient is written by bwd_masked_iou_kernel (masked groups), by the two grad_iou loops of solve_groups_kernel<true, false>
(unmasked groups: one wave per group up to 16 members, one workgroup per group above, tiled in LDS up to 128 members) and by
ungrouped_grad_iou_kernel; all of them read what the forward pass left in the workspace, and the forward pass fills the workspace by
a different launch sequence per size, per symmetry of the thresholded matrix and per mode (csrc/nms_layer.hip::forward_matrix; the route
of every case below is listed in LABNOTES R12).  The oracle's own matrix gradient is pinned against float64 autograd in
tests/test_grad_iou_host.py, whose case generator and asymmetric perturbation are used here.

Masked groups with linear pruning: bit-identical -- the kernel computes (-(gx * s_head)) * d, the oracle -(gx * s_head) and then * d, two
fp32 products with nothing to contract.  Everything else: atol 5e-4, rtol 1e-3, the suite's tolerance for grad_iou against the oracle
(test_gpu_parity.py::test_random_vs_oracle).  Always: the non-zero pattern equals the oracle's (an entry at the transposed position is a
different entry), prob and grad_scores are compared in the same call, and a second backward from a fresh forward gives the same bits.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import MODES, TOL, check_index_lists
from test_grad_iou_host import DEFAULTS, HOST_CASES, SEED, clustered_case, f64_layer

pytestmark = pytest.mark.gpu

SYM = pytest.mark.parametrize("asym", [False, True], ids=["sym", "asym"])


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


@functools.lru_cache(maxsize=2)
def _case(seed, n, per, asym):
    from oracle import oracle
    s, m, w = clustered_case(oracle, seed, n, per, asym)
    for a in (s, m, w):
        a.setflags(write=False)
    if asym:
        thr = np.float32(0.4)
        assert ((m > thr) != (m > thr).T).any(), "the perturbation left the thresholded matrix symmetric"
    return s, m, w


def _full(kw):
    k = dict(DEFAULTS)
    k.update(kw)
    return k


def _gpu(G, s, m, w, kw, presorted=False):
    """one forward + backward with the matrix as a leaf: dict(prob, valid, invalid, grad_scores (ndarrays), grad_iou (device tensor))"""
    st = torch.tensor(s, device="cuda").requires_grad_(True)          # (copies: the cached case arrays are read-only)
    mt = torch.tensor(m, device="cuda").requires_grad_(True)
    wt = torch.tensor(w, device="cuda")
    if presorted:
        prob, _, valid, invalid, nv, ni = G.differentiable_nms_batched(st[None], mt[None], presorted=True, **kw)
        prob, valid, invalid = prob[0], valid[0, :int(nv[0])], invalid[0, :int(ni[0])]
    else:
        valid, invalid, prob = G.differentiable_nms(st, mt, **kw)
    (prob * wt).sum().backward()
    assert mt.grad is not None and tuple(mt.grad.shape) == m.shape
    return dict(prob=prob.detach().cpu().numpy(), valid=valid.cpu().numpy(), invalid=invalid.cpu().numpy(),
                grad_scores=st.grad.cpu().numpy(), grad_iou=mt.grad)


def _close(got, ref):
    return np.abs(got - ref) <= 5e-4 + 1e-3 * np.abs(ref)


def _compare(res, ref, exact, tag, f64=None, head_sum_in_rank_order=False):
    """res: _gpu's dict (grad_iou already an ndarray); ref: the oracle's.  f64: callable giving the float64 restatement's dict, for the
    arbitration of a big-group case outside the tolerance (accepted only if the GPU's error is at most twice the oracle's own).
    head_sum_in_rank_order (masked groups, pre-sorted): dL/ds_head = gx_head - sum_i P_i gx_i is summed by bwd_masked_heads_kernel in
    the order of the members' scores, by the oracle's matmul row in the order of their input indices -- the same with hard-sorted
    scores, two associations of one fp32 sum with pre-sorted ones.  grad_scores then takes the suite's gradient tolerance; prob, the
    index lists and the matrix gradient (products of gx and s_head, no sum) stay bit-exact."""
    gi, gi_ref = res["grad_iou"], ref["grad_iou"]
    assert gi.shape == gi_ref.shape and np.isfinite(gi).all(), tag
    if exact:
        assert np.array_equal(res["prob"], ref["prob"]), f"{tag}: prob not bit-exact"
        if head_sum_in_rank_order:
            print("%s: max |grad_scores - oracle| %.3e" % (tag, float(np.abs(res["grad_scores"] - ref["grad_scores"]).max())))
            np.testing.assert_allclose(res["grad_scores"], ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=tag)
        else:
            assert np.array_equal(res["grad_scores"], ref["grad_scores"]), f"{tag}: grad_scores not bit-exact"
        assert list(res["valid"]) == list(ref["valid"]) and list(res["invalid"]) == list(ref["invalid"]), tag
    else:
        np.testing.assert_allclose(res["prob"], ref["prob"], atol=TOL, err_msg=tag)
        np.testing.assert_allclose(res["grad_scores"], ref["grad_scores"], atol=5e-4, rtol=1e-3, err_msg=tag)
        check_index_lists(res["valid"], res["invalid"], ref["valid"], ref["invalid"])
    nz, nz_ref = np.flatnonzero(gi), np.flatnonzero(gi_ref)
    assert len(nz_ref) > 0, f"{tag}: the case has no matrix gradient at all"
    if not np.array_equal(nz, nz_ref):
        extra, missing = np.setdiff1d(nz, nz_ref), np.setdiff1d(nz_ref, nz)
        n = gi.shape[-1]
        raise AssertionError(f"{tag}: non-zero pattern differs from the oracle's: {len(extra)} extra (first {[divmod(int(e), n) for e in extra[:4]]}), "
                             f"{len(missing)} missing (first {[divmod(int(e), n) for e in missing[:4]]}) of {len(nz_ref)}")
    d = np.abs(gi - gi_ref)
    print("%s: nnz %d, max |grad_iou - oracle| %.3e" % (tag, len(nz_ref), float(d.max())))
    if exact:
        bad = np.flatnonzero(gi != gi_ref)
        assert len(bad) == 0, (f"{tag}: grad_iou not bit-exact at {len(bad)} of {len(nz_ref)} entries, first "
                               f"{divmod(int(bad[0]), gi.shape[-1])}: {gi.flat[bad[0]]!r} against {gi_ref.flat[bad[0]]!r}")
        return
    ok = _close(gi, gi_ref)
    if ok.all():
        return
    assert f64 is not None, f"{tag}: grad_iou outside 5e-4 + 1e-3 |ref| at {int((~ok).sum())} entries, max |d| {float(d.max()):.3e}"
    want = f64()["grad_iou"]
    e_gpu, e_oracle = float(np.abs(gi - want).max()), float(np.abs(gi_ref - want).max())
    print("%s: float64 arbitration: GPU %.3e, oracle %.3e" % (tag, e_gpu, e_oracle))
    assert e_gpu <= 2.0 * e_oracle, f"{tag}: against float64 the GPU is off by {e_gpu:.3e}, the oracle by {e_oracle:.3e}"


def _run_single(G, O, s, m, w, kw, presorted, exact, tag, big_groups=False):
    k = _full(kw)
    ref = O._nms_core(s, m, w, True, 1 if presorted else 0, **k)
    res = _gpu(G, s, m, w, kw, presorted)
    again = _gpu(G, s, m, w, kw, presorted)["grad_iou"]
    assert torch.equal(res["grad_iou"], again), f"{tag}: a second backward from a fresh forward gives another matrix gradient"
    del again
    res["grad_iou"] = res["grad_iou"].cpu().numpy()
    f64 = (lambda: f64_layer(O, s, m, w, presorted=1 if presorted else 0, oracle_result=ref, **kw)) if big_groups else None
    _compare(res, ref, exact, tag, f64, head_sum_in_rank_order=bool(presorted))
    return res, ref


# ---- 1. the forward routes, default (masked) mode ------------------------------------------------------------------------------------
# n = 1000: one launch; 1100: two super-blocks, three launches; 2112: past the 2048-key sort; 4160: past 4096.  The asymmetric matrix
# fails the device's symmetry check and takes the general scan.
@pytest.mark.parametrize("mode", ["gm_lin", "gm_lin_sorted", "gm_sig"])
@SYM
@pytest.mark.parametrize("n", [1000, 1100, 2112, 4160])
def test_forward_routes_masked(G, O, n, asym, mode):
    s, m, w = _case(1300 + n, n, 32, asym)
    _run_single(G, O, s, m, w, MODES[mode], False, mode.startswith("gm_lin"), f"n={n} {'asym' if asym else 'sym'} {mode}")


# ---- 2. masked, pre-sorted: what sorting_method="soft" feeds the layer ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gm_lin", "gm_lin_sorted", "gm_lin_thr", "gm_sig"])
@SYM
@pytest.mark.parametrize("n", [1100, 2112])
def test_masked_presorted(G, O, n, asym, mode):
    s, m, w = _case(1400 + n, n, 32, asym)
    assert not (s[:-1] >= s[1:]).all(), "the scores must not be descending: the kernels have to honour the flag, not re-sort"
    res, ref = _run_single(G, O, s, m, w, MODES[mode], True, mode.startswith("gm_lin"), f"presorted n={n} {'asym' if asym else 'sym'} {mode}")
    assert not np.triu(res["grad_iou"], 1).any(), "pre-sorted: P = tril(...) kills every entry above the diagonal"
    assert np.tril(res["grad_iou"], -1).any()


# ---- 3. unmasked groups on the wave path (groups of 2-16 from the matrix) --------------------------------------------------------------
@pytest.mark.parametrize("mode,asym", [("gu_lin", False), ("gu_lin", True), ("gu_sig", False)], ids=["gu_lin-sym", "gu_lin-asym", "gu_sig-sym"])
@pytest.mark.parametrize("n", [1100, 4160])
def test_unmasked_wave_path(G, O, n, mode, asym):
    s, m, w = _case(1500 + n, n, 4, asym)
    sizes = np.array([len(g) for g in O.get_groups(m, 0.4, s, 100)])
    wave, big = int(((sizes >= 2) & (sizes <= 16)).sum()), int((sizes > 16).sum())
    # n = 1100: the wave path alone.  n = 4160: 1040 clusters on the same canvas overlap one another, and with every seed tried a handful
    # of groups (8 of ~790 here, at most 27 members) go to the tiled workgroup path beside the wave path's
    assert wave >= 250 and (big == 0 if n == 1100 else big <= wave // 50), f"{wave} groups of 2-16, {big} above (largest {sizes.max()})"
    _run_single(G, O, s, m, w, MODES[mode], False, False, f"wave n={n} {'asym' if asym else 'sym'} {mode}")


# ---- 4. unmasked groups on the workgroup path: tiled (17-128 members) and untiled (above 128) -----------------------------------------
BIG = [c for c in HOST_CASES if c[0].startswith("gu_")]


@SYM
@pytest.mark.parametrize("case", BIG, ids=[c[0] for c in BIG])
def test_unmasked_big_groups(G, O, case, asym):
    tag, n, per, kw, _ = case
    s, m, w = _case(SEED[tag], n, per, asym)
    _run_single(G, O, s, m, w, kw, False, False, f"{tag} {'asym' if asym else 'sym'}", big_groups=True)


@SYM
def test_unmasked_big_groups_presorted(G, O, asym):
    """pre-sorted scores put every multi-member group on the workgroup path, which re-slots the members by input index"""
    tag, n, per, kw, _ = BIG[0]
    s, m, w = _case(SEED[tag], n, per, asym)
    res, _ = _run_single(G, O, s, m, w, kw, True, False, f"{tag} presorted {'asym' if asym else 'sym'}", big_groups=True)
    assert not np.triu(res["grad_iou"], 1).any()


@SYM
def test_unmasked_big_and_small_groups_share_a_launch(G, O, asym):
    """n = 1100, per = 150: groups above 128 members (the second list at the end of hlist) beside groups of 2-16 (the wave path)"""
    kw = BIG[0][3]
    s, m, w = _case(1600, 1100, 150, asym)
    sizes = [len(g) for g in O.get_groups(m, 0.4, s, kw["group_size"])]
    assert max(sizes) > 128 and any(2 <= x <= 16 for x in sizes), sorted(sizes)[-8:]
    _run_single(G, O, s, m, w, kw, False, False, f"big+small n=1100 {'asym' if asym else 'sym'}", big_groups=True)


# ---- 5. ungrouped, ragged batch: the whole [N, N] of every image -----------------------------------------------------------------------
def _batch(seed, B, N, per, pad=0):
    """scores [B,N], matrix [B,N,N] as a view of a [B,N,N+pad] buffer, w [B,N]; images are the clustered cases seed + b"""
    from oracle import oracle
    parts = [clustered_case(oracle, seed + b, N, per, False) for b in range(B)]
    buf = np.full((B, N, N + pad), 0.77, np.float32)                   # (the buffer's padding columns hold a value above every threshold)
    for b in range(B):
        buf[b, :, :N] = parts[b][1]
    return np.stack([p[0] for p in parts]), buf, np.stack([p[2] for p in parts])


def _run_batched(G, scores, buf, w, counts, kw):
    """differentiable_nms_batched on the [:, :, :N] view of buf -> prob, grad_scores, grad_iou as ndarrays"""
    N = scores.shape[1]
    st = torch.from_numpy(scores).cuda().requires_grad_(True)
    mt = torch.from_numpy(buf).cuda()[:, :, :N].requires_grad_(True)
    assert mt.stride(1) == buf.shape[2]
    prob = G.differentiable_nms_batched(st, mt, counts=torch.from_numpy(np.asarray(counts, np.int32)).cuda(), **kw)[0]
    (prob * torch.from_numpy(w).cuda()).sum().backward()
    assert tuple(mt.grad.shape) == (scores.shape[0], N, N)
    return prob.detach().cpu().numpy(), st.grad.cpu().numpy(), mt.grad.cpu().numpy()


def _check_batched(O, got, scores, buf, w, counts, kw, exact, tag):
    prob, gs, gi = got
    N = scores.shape[1]
    assert gi.shape == (len(counts), N, N)
    for b, n in enumerate(counts):
        t = f"{tag} image {b} n={n}"
        assert not gi[b, n:, :].any() and not gi[b, :, n:].any(), f"{t}: the padding of grad_iou is not zero"
        assert not gs[b, n:].any() and not prob[b, n:].any(), t
        if n == 0:
            assert not gi[b].any()
            continue
        ref = O._nms_core(scores[b, :n], np.ascontiguousarray(buf[b, :n, :n]), w[b, :n], True, 0, **_full(kw))
        if n == 1:
            assert not ref["grad_iou"].any() and not gi[b].any(), t
            assert np.array_equal(prob[b, :1], ref["prob"]) and np.array_equal(gs[b, :1], ref["grad_scores"]), t
            continue
        res = dict(prob=prob[b, :n], grad_scores=gs[b, :n], grad_iou=gi[b, :n, :n], valid=ref["valid"], invalid=ref["invalid"])
        _compare(res, ref, exact, t)


@pytest.mark.parametrize("mode", ["un_lin", "un_sig"])
def test_ungrouped_ragged_whole_matrix(G, O, mode):
    counts = [300, 129, 1, 0]
    scores, buf, w = _batch(1700, 4, 300, 24)
    got = _run_batched(G, scores, buf, w, counts, MODES[mode])
    _check_batched(O, got, scores, buf, w, counts, MODES[mode], False, mode)
    assert np.array_equal(got[2], _run_batched(G, scores, buf, w, counts, MODES[mode])[2]), "a second run gives another matrix gradient"


# ---- 6. batched, ragged, strided (ld = N + 7), through both bindings ---------------------------------------------------------------------
STRIDED_COUNTS = [260, 0, 77]
STRIDED_MODES = ["gm_lin", "gu_lin", "un_lin"]


def _strided_run(G):
    scores, buf, w = _batch(1800, 3, 260, 20, pad=7)
    return {mode: _run_batched(G, scores, buf, w, STRIDED_COUNTS, MODES[mode]) for mode in STRIDED_MODES}, (scores, buf, w)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, "tests")
import groomed_nms_amd as G
from groomed_nms_amd import groomed_nms as GN
import test_grad_iou_routes as T
assert not GN._binding()
out, _ = T._strided_run(G)
np.savez(sys.argv[1], **{m + "/" + k: v for m, r in out.items() for k, v in zip(("prob", "gs", "gi"), r)})
"""


def test_batched_ragged_strided_both_bindings(G, O):
    from groomed_nms_amd import groomed_nms as GN
    assert GN._binding(), "the C++ binding is not in use in this process"
    out, (scores, buf, w) = _strided_run(G)
    for mode in STRIDED_MODES:
        assert out[mode][2].shape == (3, 260, 260)
        assert not out[mode][2][1].any(), f"{mode}: the empty image has a matrix gradient"
        _check_batched(O, out[mode], scores, buf, w, STRIDED_COUNTS, MODES[mode], mode == "gm_lin", f"ld=267 {mode}")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ctypes.npz")
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _CHILD, path], cwd=root, env=dict(os.environ, GNMS_BINDING="ctypes"),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        child = np.load(path)
        for mode in STRIDED_MODES:
            for k, v in zip(("prob", "gs", "gi"), out[mode]):
                assert np.array_equal(v, child[f"{mode}/{k}"]), f"{mode}/{k}: the ctypes path and the C++ binding differ"
