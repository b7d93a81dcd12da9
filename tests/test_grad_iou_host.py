"""The CPU oracle's dL/d(overlap matrix) against a float64 restatement of the layer that autograd differentiates.

tests/test_grad_iou_routes.py takes oracle._nms_core(..., want_grad_iou=True) as the reference for the HIP kernels' matrix
gradient in regimes no golden vector holds: groups above 16 and above 128 members, a non-linear f', a thresholded and sorted
return, pre-sorted input, an asymmetric matrix, the ungrouped inverse.  This file pins the oracle there first.  `f64_layer` is
lib/groomed_nms.py:41-127 in float64 torch on the CPU, with torch.linalg.inv where the reference inverts, and torch.autograd for
the gradient: it shares no closed form with csrc/nms_backward_kernels.h or with the backward of oracle/gnms_oracle.c.

Every DECISION is taken from the fp32 run, so that no threshold is re-taken in another precision: the score order (argsort of the
fp32 scores), the groups (oracle.get_groups on the fp32 matrix) and, for return_sorted_prob, the order of the returned
probabilities (the oracle's valid + invalid lists; checked to be descending in float64 too).  Three decisions remain that depend
on a computed value: the two clamp bounds and valid_box_prob_threshold.  A box whose float64 pre-clamp value is within 1e-5 of 0
or 1 (exact zeros apart: the all-zero rows of M, boxes in no group, are zero in every precision and take no part in anything), or,
where the thresholded tensor is returned, within 1e-5 of the threshold, is left out of the comparison -- together with whatever its
gx reaches: its head (masked groups), its group (unmasked); in the ungrouped mode there must be none.  At most 1 % of a case's
boxes may be left out; the committed seeds have none (LABNOTES R12).

E_REF holds, per case, the largest difference of the oracle from the restatement as measured when the seeds were chosen
(LABNOTES R12); the assertion is e <= 4 * e_ref -- both sides are deterministic host code, the factor absorbs another libm or LAPACK.
"""
import numpy as np
import pytest
import torch

NEAR = 1e-5            # a decision within this of its bound is not compared
REL_FLOOR = 1e-3       # relative differences are taken where |reference| >= this; below it the absolute figure governs

# (tag, n, per, keywords of the layer, presorted)
HOST_CASES = [
    ("gu_big149", 300, 150, dict(mask_group_boxes=False, group_size=500), 0),
    ("gu_cap121", 300, 150, dict(mask_group_boxes=False, group_size=120), 0),
    ("gu_sig_gs40", 300, 150, dict(mask_group_boxes=False, group_size=40, pruning_method="sigmoidal", temperature=0.1), 0),
    ("gm_sorted", 1100, 32, dict(return_sorted_prob=True), 0),
    ("gm_presorted", 1100, 32, dict(), 1),
    ("un_272", 272, 8, dict(group_boxes=False), 0),
]
SEED = {c[0]: 1200 for c in HOST_CASES}      # chosen so that no box of any case, symmetric or not, is left out (checked on the CPU)

DEFAULTS = dict(nms_threshold=0.4, pruning_method="linear", temperature=0.01, valid_box_prob_threshold=0.3, return_sorted_prob=False,
                group_boxes=True, mask_group_boxes=True, group_size=100)


def asymmetric(m, rng):
    """the strict upper triangle times fp32 factors from U(0.8, 1.2), clipped to [0, 1]"""
    f = rng.uniform(0.8, 1.2, size=m.shape).astype(np.float32)
    out = m.copy()
    iu = np.triu_indices(m.shape[0], 1)
    out[iu] = np.clip(out[iu] * f[iu], np.float32(0.0), np.float32(1.0))
    return out


def clustered_case(O, seed, n, per, asym):
    """(scores, matrix, w) fp32: clustered boxes, tie-free scores, w ~ U(-1, 2); the asymmetric form perturbs the same matrix"""
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    b = synthetic.clustered_boxes_2d(rng, n, per)
    s = synthetic.tie_free_scores(rng, n)
    w = rng.uniform(-1, 2, size=n).astype(np.float32)
    m = O.iou2d(b, b)
    if asym:
        m = asymmetric(m, rng)
    return s, m, w


def _prune64(x, thr, temp, method):
    if method == "linear":
        return x
    if method == "sigmoidal":
        return torch.sigmoid((x - thr) / temp)
    return 1.0 - torch.exp(-(x * x) / temp)


def f64_layer(O, scores, iou, w, presorted=0, oracle_result=None, **kw):
    """float64 restatement + autograd.  Returns dict(prob, grad_scores, grad_iou (input order, float64 ndarrays), pre (by NMS
    position), order, groups (lists of NMS positions))."""
    k = dict(DEFAULTS)
    k.update(kw)
    # the parameters as the fp32 layer sees them
    thr, temp, vthr = (float(np.float32(k[x])) for x in ("nms_threshold", "temperature", "valid_box_prob_threshold"))
    n = len(scores)
    order = np.arange(n) if presorted else O.argsort_desc(scores)
    ot = torch.from_numpy(np.asarray(order, np.int64))
    s = torch.tensor(np.asarray(scores, np.float64), requires_grad=True)
    m = torch.tensor(np.asarray(iou, np.float64), requires_grad=True)
    ss = s[ot]
    mm = m[ot][:, ot]
    P = torch.tril(_prune64(mm, thr, temp, k["pruning_method"]), -1)
    eye = torch.eye(n, dtype=torch.float64)
    groups = []
    if k["group_boxes"]:
        s32 = np.ascontiguousarray(np.asarray(scores, np.float32)[order])
        m32 = np.ascontiguousarray(np.asarray(iou, np.float32)[np.ix_(order, order)])
        groups = [g for g in O.get_groups(m32, k["nms_threshold"], s32, k["group_size"]) if len(g)]
        if k["mask_group_boxes"]:
            mask = torch.zeros((n, n), dtype=torch.float64)
            member = torch.zeros(n, dtype=torch.float64)
            for g in groups:
                mask[torch.from_numpy(g), int(g[0])] = 1.0
                member[torch.from_numpy(g)] = 1.0
            M = torch.diag(member) - P * mask
        else:
            M = torch.zeros((n, n), dtype=torch.float64)
            for g in groups:
                gt = torch.from_numpy(g)
                blk = torch.linalg.inv(torch.eye(len(g), dtype=torch.float64) + P[gt][:, gt])
                M = M.index_put((gt[:, None].expand(-1, len(g)), gt[None, :].expand(len(g), -1)), blk)
    else:
        M = torch.linalg.inv(eye + P)
    pre = M @ ss
    r2 = torch.clamp(pre, 0.0, 1.0)
    r = r2 * (r2.detach() >= vthr).to(torch.float64)                 # zeroed in place below the threshold
    thresholded = bool(k["return_sorted_prob"]) or not k["group_boxes"]
    if k["return_sorted_prob"]:
        # the order of the returned probabilities is the fp32 run's: rank -> NMS position, from its two index lists
        assert oracle_result is not None
        pos_of = np.empty(n, np.int64)
        pos_of[order] = np.arange(n)
        sidx = pos_of[np.concatenate([oracle_result["valid"], oracle_result["invalid"]])]
        assert len(sidx) == n and len(np.unique(sidx)) == n
        prob = r[torch.from_numpy(sidx)]
        assert bool((prob.detach()[:-1] - prob.detach()[1:] >= -1e-6).all()), "the fp32 order is not descending in float64"
    else:
        prob = r2 if k["group_boxes"] else r
    (prob * torch.tensor(np.asarray(w, np.float64))).sum().backward()
    return dict(prob=prob.detach().numpy(), grad_scores=s.grad.numpy(), grad_iou=m.grad.numpy(), pre=pre.detach().numpy(),
                r2=r2.detach().numpy(), order=np.asarray(order), groups=[np.asarray(g) for g in groups], thresholded=thresholded,
                vthr=vthr, mode=("ungrouped" if not k["group_boxes"] else "masked" if k["mask_group_boxes"] else "unmasked"))


def left_out(f):
    """(number of undecided boxes, bool mask over INPUT indices of the boxes to leave out of a comparison with f)"""
    pre, r2 = f["pre"], f["r2"]
    und = ((np.abs(pre) < NEAR) & (pre != 0.0)) | ((np.abs(pre - 1.0) < NEAR) & (pre != 1.0))
    if f["thresholded"]:
        und |= np.abs(r2 - f["vthr"]) < NEAR
    out = und.copy()
    for g in f["groups"]:
        if und[g].any():
            if f["mode"] == "masked":
                out[g[0]] = True
            else:
                out[g] = True
    if f["mode"] == "ungrouped" and und.any():
        out[:] = True
    mask = np.zeros(len(pre), bool)
    mask[f["order"][out]] = True
    return int(und.sum()), mask


def errors(got, ref, skip=None):
    """(largest absolute difference, largest relative difference where |ref| >= REL_FLOOR); rows / columns in `skip` left out"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if skip is not None and skip.any():
        keep = ~skip
        got, ref = (got[keep], ref[keep]) if got.ndim == 1 else (got[np.ix_(keep, keep)], ref[np.ix_(keep, keep)])
    d = np.abs(got - ref)
    big = np.abs(ref) >= REL_FLOOR
    return float(d.max()) if d.size else 0.0, float((d[big] / np.abs(ref[big])).max()) if big.any() else 0.0


def run_case(O, tag, n, per, kw, presorted, asym):
    s, m, w = clustered_case(O, SEED[tag], n, per, asym)
    k = dict(DEFAULTS)
    k.update(kw)
    ref = O._nms_core(s, m, w, True, presorted, **k)
    f = f64_layer(O, s, m, w, presorted=presorted, oracle_result=ref, **kw)
    n_und, skip = left_out(f)
    return s, m, w, ref, f, n_und, skip


# e_ref, measured (LABNOTES R12): tag, asym -> (grad_scores abs, rel, grad_iou abs, rel)
E_REF = {
    ("gu_big149", False): (4.23e-07, 3.38e-05, 4.92e-07, 3.38e-05),   # left out 0, nnz 21904, largest groups [150, 150]
    ("gu_big149", True): (8.27e-07, 3.66e-05, 7.49e-07, 3.67e-05),   # left out 0, nnz 22201, largest groups [150, 149, 1]
    ("gu_cap121", False): (4.37e-07, 1.90e-06, 4.15e-07, 3.01e-05),   # left out 0, nnz 14520, largest groups [121, 121]
    ("gu_cap121", True): (6.81e-07, 5.57e-06, 6.23e-07, 2.17e-05),   # left out 0, nnz 14280, largest groups [121, 121, 1]
    ("gu_sig_gs40", False): (6.15e-07, 1.93e-05, 1.14e-06, 2.58e-05),   # left out 0, nnz 1600, largest groups [41, 41]
    ("gu_sig_gs40", True): (7.15e-07, 2.56e-05, 1.45e-06, 9.42e-05),   # left out 0, nnz 1640, largest groups [41, 41, 1]
    ("gm_sorted", False): (1.37e-07, 1.83e-06, 5.84e-08, 5.32e-08),   # left out 0, nnz 69, largest groups [33, 33, 33]
    ("gm_sorted", True): (1.56e-07, 1.52e-07, 5.65e-08, 5.33e-08),   # left out 0, nnz 75, largest groups [33, 33, 33]
    ("gm_presorted", False): (1.75e-07, 8.06e-07, 5.90e-08, 5.49e-08),   # left out 0, nnz 201, largest groups [33, 33, 33]
    ("gm_presorted", True): (1.75e-07, 8.06e-07, 5.90e-08, 5.49e-08),   # left out 0, nnz 201, largest groups [33, 33, 33]
    ("un_272", False): (4.34e-08, 1.03e-07, 1.20e-07, 3.29e-06),   # left out 0, nnz 1631, largest groups []
    ("un_272", True): (4.34e-08, 1.03e-07, 8.76e-08, 3.53e-06),   # left out 0, nnz 1624, largest groups []
}


@pytest.mark.parametrize("asym", [False, True], ids=["sym", "asym"])
@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_oracle_matrix_gradient_against_float64_autograd(case, asym):
    from oracle import oracle as O
    tag, n, per, kw, presorted = case
    s, m, w, ref, f, n_und, skip = run_case(O, tag, n, per, kw, presorted, asym)
    assert n_und <= n // 100, f"{tag}: {n_und} of {n} boxes sit within {NEAR} of a clamp bound or the threshold"
    if f["mode"] == "ungrouped":
        assert n_und == 0, f"{tag}: an undecided box reaches every gradient of the ungrouped mode"
    if asym:
        thr = np.float32(DEFAULTS["nms_threshold"])
        assert ((m > thr) != (m > thr).T).any(), "the perturbation left the thresholded matrix symmetric"
    else:
        assert np.array_equal(m, m.T)
    np.testing.assert_allclose(ref["prob"], f["prob"], atol=1e-5, rtol=0, err_msg=tag)
    gi, gi64 = ref["grad_iou"], f["grad_iou"]
    # the sparsity pattern is part of the result: an entry at the transposed position is a different entry
    keep = ~skip
    assert np.array_equal((gi != 0)[np.ix_(keep, keep)], (gi64 != 0)[np.ix_(keep, keep)]), f"{tag}: non-zero pattern differs"
    if presorted:
        assert not np.triu(gi, 1).any() and not np.triu(gi64, 1).any(), "pre-sorted: the strict upper triangle must be exactly zero"
    e = errors(ref["grad_scores"], f["grad_scores"], skip) + errors(gi, gi64, skip)
    print("e_ref %-14s %-4s n_left_out=%d nnz=%d  grad_scores abs %.3e rel %.3e  grad_iou abs %.3e rel %.3e"
          % (tag, "asym" if asym else "sym", n_und, int((gi != 0).sum()), *e))
    # the GPU tests compare with the oracle at 5e-4 + 1e-3 |ref|: an oracle outside that would be a finding about the oracle
    for got, want in ((ref["grad_scores"], f["grad_scores"]), (gi, gi64)):
        assert (np.abs(got - want) <= 5e-4 + 1e-3 * np.abs(want))[keep if got.ndim == 1 else np.ix_(keep, keep)].all(), tag
    bound = E_REF[(tag, asym)]
    assert all(x <= 4.0 * b for x, b in zip(e, bound)), f"{tag}: {e} against 4 x e_ref = {bound}"
