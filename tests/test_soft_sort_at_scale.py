"""soft_sort (lib/groomed_nms.py:131-165) and differentiable_nms(sorting_method="soft") past 300 boxes, where the soft sort's kernels change
shape: the larger in-LDS sorts (sort_scores_kernel<2/4/8/16>, the > 64 KiB LDS attribute), the vendor products behind launch_sgemm (rocBLAS
from 512^3, hipBLASLt from 2048^3, with and without accumulation, padded leading dimensions), the products under stream capture (the
library's own split-K kernels), concurrent streams, and the layer in presorted mode at scale.

The reference is a plain float64 evaluation of the reference's own expressions (:145-164) on the GPU, its backward float64 autograd of the
same graph; the layer stage is the C oracle (oracle._nms_core on the GPU's own soft scores / soft matrix, chained with
oracle._soft_sort_backward).  Tolerances are element-wise forward-error bounds, stated where they are built:
  * a product D = A B over K terms: |D - A B| <= 2 K u (|A| |B|), u = 2^-24, against float64 of the GPU's own fp32 operands;
  * the convex-combination matrix C: the rounding of the fp32 expression, propagated element by element (_c_bound);
  * gradients: the gradient-scale form of test_gpu_parity._assert_grad_close.
A dropped accumulation, a transposed operand or a wrong leading dimension miss these bounds by orders of magnitude."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from conftest import TOL, check_index_lists
from test_gpu_parity import _assert_grad_close, _record

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # unit roundoff of fp32
GRAD_TOL = 5e-6          # gradients, in units of the gradient's own scale (_assert_grad_close); measured on the MI355X: <= 1.7e-6 (N = 4096, T = 1)
LOG = "soft_sort_at_scale.jsonl"


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


@pytest.fixture(scope="module")
def backends(G):
    """which vendor libraries launch_sgemm can reach in this process: a 64^3 product through gnms_profile_sgemm at variant 2 (rocBLAS
    only) and 4 (hipBLASLt only); a missing library refuses with GNMS_ERR_UNSUPPORTED"""
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    a = torch.ones((64, 64), device="cuda")
    got = {}
    for variant, name in ((2, "rocBLAS"), (4, "hipBLASLt")):
        d = torch.zeros((64, 64), device="cuda")
        rc = lib.gnms_profile_sgemm(ptr(a), ptr(a), ptr(d), 64, 64, 64, 64, 64, 64, variant, stream_ptr())
        torch.cuda.synchronize()
        got[name] = bool(rc == 0 and torch.all(d == 64.0))
    _record(LOG, {"backends": got})
    return got


def _ctx(backends, **kw):
    return " ".join([f"{k}={v}" for k, v in kw.items()] + ["vendor libraries reachable: %s" % backends])


def _within(got, ref, bound, tag, ctx):
    """element-wise |got - ref| <= bound (NaN anywhere fails)"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    worst = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    _record(LOG, {"what": tag, "worst_err_over_bound": worst})
    assert bool(ok.all()), f"{tag}: {int((~ok).sum())} of {err.numel()} elements outside the bound, worst err / bound = {worst:.3g}; {ctx}"


def _product_bound(a, b, K, c=2.0):
    """forward-error bound of an fp32 product over K terms, from its float64 operands"""
    return c * max(K, 1) * U * (a.abs() @ b.abs())


def _reference(s32, m32, T, gs=None, gC=None, gm=None):
    """float64 evaluation of lib/groomed_nms.py:145-164 on the GPU: shat by a stable descending sort (the library's tie rule: equal scores,
    -0.0 and +0.0 included, keep input order -- the reference's torch.sort leaves ties unspecified); C[i][j] = E[i][j] / Z[j] (the last-axis
    broadcast of :155).  With upstream gradients: float64 autograd of the same graph.  T as the fp32 value the kernels receive."""
    T64 = float(np.float32(T))
    want = gs is not None or gC is not None or gm is not None
    s = s32.detach().double().requires_grad_(want)
    m = m32.detach().double().requires_grad_(want) if m32 is not None else None
    order = torch.from_numpy(np.argsort(-s32.detach().cpu().numpy(), kind="stable")).to(s.device)
    shat = s[order]
    A = -(s.unsqueeze(0) - shat.unsqueeze(1)).abs()
    arg = (A - A.max(dim=1, keepdim=True)[0]) / T64
    E = torch.exp(arg)
    Z = E.sum(dim=1) + 1e-3
    C = E / Z
    ss = C @ s
    sm = C @ m if m is not None else None
    out = dict(C=C.detach(), ss=ss.detach(), sm=sm.detach() if sm is not None else None, arg=arg.detach(), E=E.detach(), Z=Z.detach())
    if want:
        loss = 0.0
        if gs is not None:
            loss = loss + (ss * gs.double()).sum()
        if gC is not None:
            loss = loss + (C * gC.double()).sum()
        if gm is not None:
            loss = loss + (sm * gm.double()).sum()
        loss.backward()
        out["d_scores"] = s.grad
        out["d_matrix"] = m.grad if m is not None else None
    return out


def _c_bound(ref, N):
    """forward-error bound of the fp32 C = E / Z[j]: the kernel's argument (-|s_j - shat_i| - 0) / T rounds twice (2 u |arg|), expf adds
    <= 4 u; Z[i] sums the row's rounded E (their weighted error) in <= N/256 + 10 fp32 additions; the division adds u.  Factor 2 on top;
    2^-125 absolute below the normal range (where expf and the division lose relative precision)."""
    arg, E, Z, C = ref["arg"], ref["E"], ref["Z"], ref["C"]
    relE = U * (2.0 * arg.abs() + 4.0)
    relZ = (E * relE).sum(dim=1) / Z + U * (N / 256.0 + 10.0)
    return 2.0 * (relE + relZ.unsqueeze(0) + U) * C + 2.0 ** -125


def _check_forward(ref, C, ss, sm, m32, s32, N, tag, ctx):
    _within(C, ref["C"], _c_bound(ref, N), f"{tag} C", ctx)
    C64 = C.double()
    _within(ss, C64 @ s32.double(), _product_bound(C64, s32.double().unsqueeze(1), N).squeeze(1), f"{tag} soft_scores", ctx)
    if sm is not None:
        m64 = m32.double()
        _within(sm, C64 @ m64, _product_bound(C64, m64, N), f"{tag} soft_matrix", ctx)


def _rand(rng, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(lo, hi, size=shape).astype(np.float32)).cuda()


def _uniform_scores(rng, n):
    from groomed_nms_amd import synthetic
    return torch.from_numpy(synthetic.tie_free_scores(rng, n)).cuda()


# ------------------------------------------------------------------------------------------------------------------------------------------
def test_vendor_libraries_are_reachable(backends):
    """the tests below exercise the rocBLAS and hipBLASLt paths of launch_sgemm only where the libraries load; on the MI355X image both do"""
    assert all(backends.values()), f"vendor libraries reachable: {backends}"


@pytest.mark.parametrize("T", [1.0, 1e-3])
def test_soft_sort_across_the_dispatch_thresholds(G, backends, T):
    """soft_sort forward and backward with all three upstream gradients (g_soft, g_C, g_mat), asymmetric matrices, unsorted scores.
    Square N crosses the product's thresholds (own kernels < 512^3 <= rocBLAS < 2048^3 <= hipBLASLt): the forward C M, the accumulating
    dC += g_mat M^T (beta = 1, C = D on the library) and dM = C^T g_mat.  Rectangular K at N = 2048 moves one axis of each backward
    product across a threshold on its own (77: own kernels, 600: rocBLAS, 2100: hipBLASLt).  T = 1: dense rows; 1e-3: near one-hot."""
    rng = np.random.default_rng(int(1 / T) + 11)
    for N, K in [(n, n) for n in (300, 511, 512, 600, 1025, 2047, 2048, 2500, 4096)] + [(2048, 77), (2048, 600), (2048, 2100)]:
        ctx = _ctx(backends, N=N, K=K, T=T)
        s32 = _uniform_scores(rng, N)
        m32 = _rand(rng, (N, K))
        gs, gC, gm = _rand(rng, (N,)), _rand(rng, (N, N)), _rand(rng, (N, K))
        st, mt = s32.clone().requires_grad_(True), m32.clone().requires_grad_(True)
        ss, C, sm = G.soft_sort(st, mt, T)
        ((ss * gs).sum() + (C * gC).sum() + (sm * gm).sum()).backward()
        torch.cuda.synchronize()
        ref = _reference(s32, m32, T, gs, gC, gm)
        tag = f"N={N} K={K} T={T:g}"
        _check_forward(ref, C.detach(), ss.detach(), sm.detach(), m32, s32, N, tag, ctx)
        C64 = C.detach().double()
        _within(mt.grad, C64.t() @ gm.double(), _product_bound(C64.t(), gm.double(), N), f"{tag} d_matrix", ctx)
        _assert_grad_close(st.grad.cpu().numpy(), ref["d_scores"].cpu().numpy(), f"{tag} d_scores ({ctx})", tol=GRAD_TOL)
        del ss, C, sm, st, mt, ref
        torch.cuda.empty_cache()


def test_soft_sort_abi_with_padded_leading_dimensions(G, backends):
    """gnms_soft_sort with ld > N (the forward product's ldb) and gnms_soft_sort_backward with ld > K (the matrix and d_matrix), one odd ld
    and one a multiple of 4, on rocBLAS (N = 600) and hipBLASLt (N = 2048) sizes.  The padding of the inputs holds NaN (a product that reads
    it cannot pass), the padding of d_matrix a sentinel that must survive.  An odd ld may make hipBLASLt's heuristic refuse the shape; the
    product then goes elsewhere and must still be right."""
    from groomed_nms_amd import _lib
    from groomed_nms_amd._lib import GnmsParams, ptr, stream_ptr, check
    lib = _lib.load()
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    rng = np.random.default_rng(29)
    T = 0.05
    for N, K, pad in ((600, 600, 1), (600, 600, 4), (2048, 2100, 1), (2048, 2100, 4)):
        ldf, ldb = N + pad, K + pad
        ctx = _ctx(backends, N=N, K=K, ld_forward=ldf, ld_backward=ldb)
        tag = f"ABI N={N} K={K} ld={ldf}/{ldb}"
        s32 = _uniform_scores(rng, N)
        sq = _rand(rng, (N, N), 0.0, 1.0)
        iou = torch.full((N, ldf), float("nan"), device="cuda")
        iou[:, :N] = sq
        m32 = _rand(rng, (N, K))
        mat = torch.full((N, ldb), float("nan"), device="cuda")
        mat[:, :K] = m32
        gs, gC, gm = _rand(rng, (N,)), _rand(rng, (N, N)), _rand(rng, (N, K))
        ws = torch.empty((max(lib.gnms_workspace_bytes(1, N, ctypes.byref(P)), 256),), dtype=torch.uint8, device="cuda")
        C = torch.empty((N, N), device="cuda")
        ss = torch.empty((N,), device="cuda")
        sm = torch.empty((N, N), device="cuda")
        check(lib.gnms_soft_sort(ptr(s32), ptr(iou), N, ldf, T, ptr(C), ptr(ss), ptr(sm), ptr(ws), ws.numel(), stream_ptr()), "gnms_soft_sort")
        nb = lib.gnms_soft_sort_backward_scratch_bytes(N, K)
        scratch = torch.empty((nb,), dtype=torch.uint8, device="cuda")
        d_s = torch.empty((N,), device="cuda")
        d_m = torch.full((N, ldb), -7.0, device="cuda")
        check(lib.gnms_soft_sort_backward(ptr(s32), ptr(mat), N, K, ldb, T, ptr(C), ptr(gs), ptr(gC), ptr(gm), ptr(d_s), ptr(d_m), ptr(ws),
                                          ws.numel(), ptr(scratch), nb, stream_ptr()), "gnms_soft_sort_backward")
        torch.cuda.synchronize()
        _check_forward(_reference(s32, sq, T), C, ss, sm, sq, s32, N, tag, ctx)
        C64 = C.double()
        _within(d_m[:, :K], C64.t() @ gm.double(), _product_bound(C64.t(), gm.double(), N), f"{tag} d_matrix", ctx)
        assert bool(torch.all(d_m[:, K:] == -7.0)), f"{tag}: the padding columns of d_matrix were written; {ctx}"
        ref = _reference(s32, m32, T, gs, gC, gm)
        _assert_grad_close(d_s.cpu().numpy(), ref["d_scores"].cpu().numpy(), f"{tag} d_scores ({ctx})", tol=GRAD_TOL)
        del ws, C, sm, scratch, d_m, ref
        torch.cuda.empty_cache()


def _scores(kind, rng, n):
    if kind == "uniform":
        return torch.from_numpy(rng.uniform(size=n).astype(np.float32)).cuda()
    if kind == "ties":                                                 # 65 distinct values: runs of ~n / 65 equal scores
        return torch.from_numpy((np.round(rng.uniform(size=n) * 64) / 64).astype(np.float32)).cuda()
    s = rng.uniform(-1, 1, size=n).astype(np.float32)                  # signed, with runs of +0.0 and -0.0 spread through the input
    z = rng.choice(n, size=max(8, n // 50), replace=False)
    s[z[0::2]] = 0.0
    s[z[1::2]] = -0.0
    return torch.from_numpy(s).cuda()


@pytest.mark.parametrize("kind", ["uniform", "ties", "signed_zeros"])
def test_soft_sort_larger_sorts(G, backends, kind):
    """The score sort behind C for N > 1024: sort_scores_kernel<EE> with EE = 2 (1025), 4 (3000), 8 (5000) and 16 (8193: 128 KiB of LDS,
    the > 64 KiB attribute).  Forward without a matrix, backward with g_soft and g_C: C is wrong everywhere if a key lands in the wrong
    place, and d_scores routes dshat through the sort's rank of every index (ties: input order, as the stable reference)."""
    rng = np.random.default_rng({"uniform": 1, "ties": 2, "signed_zeros": 3}[kind])
    T = 1e-3
    for N in (1025, 3000, 5000, 8193):
        ctx = _ctx(backends, N=N, kind=kind, T=T)
        s32 = _scores(kind, rng, N)
        gs, gC = _rand(rng, (N,)), _rand(rng, (N, N))
        st = s32.clone().requires_grad_(True)
        ss, C = G.soft_sort(st, None, T)
        ((ss * gs).sum() + (C * gC).sum()).backward()
        torch.cuda.synchronize()
        ref = _reference(s32, None, T, gs, gC, None)
        tag = f"sort N={N} {kind}"
        _check_forward(ref, C.detach(), ss.detach(), None, None, s32, N, tag, ctx)
        _assert_grad_close(st.grad.cpu().numpy(), ref["d_scores"].cpu().numpy(), f"{tag} d_scores ({ctx})", tol=GRAD_TOL)
        del ss, C, st, ref
        torch.cuda.empty_cache()


SOFT_LAYER_MODES = {"default": dict(), "unmasked": dict(mask_group_boxes=False), "ungrouped": dict(group_boxes=False)}


@pytest.mark.parametrize("mode", list(SOFT_LAYER_MODES))
def test_soft_layer_at_scale(G, O, backends, mode):
    """differentiable_nms(sorting_method="soft") on clustered boxes with descending scores: soft_sort, the layer in presorted mode (tril by
    input index, the group solves' workgroup path, the backward's gx indexing and grad_iou), then the soft sort's adjoint.  The layer stage
    is the oracle's on the GPU's own soft scores and soft matrix (identical threshold inputs), its gradients chained through
    oracle._soft_sort_backward with the GPU's C.  sorting_temperature = 2e-4 keeps every case non-trivial (1e-2 leaves no valid box).
    The ungrouped mode runs at 700 and 1025 boxes only: the oracle's ungrouped solve takes 10 s at 2048."""
    from groomed_nms_amd import synthetic
    kw = SOFT_LAYER_MODES[mode]
    T = 2e-4
    for N in (700, 1025, 2048, 4096):
        if mode == "ungrouped" and N > 1025:
            continue
        ctx = _ctx(backends, N=N, mode=mode, sorting_temperature=T)
        rng = np.random.default_rng(N)
        b = synthetic.clustered_boxes_2d(rng, N, 16)
        s = np.sort(synthetic.tie_free_scores(rng, N))[::-1].copy()
        m = O.iou2d(b, b)
        w = rng.uniform(-1, 2, size=N).astype(np.float32)
        st = torch.from_numpy(s).cuda().requires_grad_(True)
        mt = torch.from_numpy(m).cuda().requires_grad_(True)
        valid, invalid, prob = G.differentiable_nms(st, mt, sorting_method="soft", sorting_temperature=T, **kw)
        (prob * torch.from_numpy(w).cuda()).sum().backward()
        ss, C, sm = G.soft_sort(torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda(), T)
        torch.cuda.synchronize()
        ss, C, sm = ss.cpu().numpy(), C.cpu().numpy(), sm.cpu().numpy()
        ref = O._nms_core(ss, sm, w, True, 1, nms_threshold=0.4, pruning_method="linear", temperature=0.01, valid_box_prob_threshold=0.3,
                          return_sorted_prob=False, group_boxes=kw.get("group_boxes", True), mask_group_boxes=kw.get("mask_group_boxes", True),
                          group_size=100)
        gs_ref, gi_ref = O._soft_sort_backward(s, m, T, C, ref["grad_scores"], ref["grad_iou"])
        assert 0 < len(ref["valid"]) < N, f"trivial case: {len(ref['valid'])} valid of {N}; {ctx}"
        got = prob.detach().cpu().numpy()
        err = float(np.abs(got - ref["prob"]).max())
        assert err <= TOL, f"probabilities: max |d| = {err:.3g}; {ctx}"
        check_index_lists(valid.cpu().numpy(), invalid.cpu().numpy(), ref["valid"], ref["invalid"])
        _assert_grad_close(st.grad.cpu().numpy(), gs_ref, f"soft layer N={N} {mode} grad_scores ({ctx})", tol=GRAD_TOL)
        _assert_grad_close(mt.grad.cpu().numpy(), gi_ref, f"soft layer N={N} {mode} grad_iou ({ctx})", tol=GRAD_TOL)


def _soft_step(G, s, m, gs, gC, gm, T):
    """soft_sort forward and backward; returns (soft_scores, C, soft_matrix, d_scores, d_matrix)"""
    st, mt = s.detach().requires_grad_(True), m.detach().requires_grad_(True)
    ss, C, sm = G.soft_sort(st, mt, T)
    ds, dm = torch.autograd.grad((ss * gs).sum() + (C * gC).sum() + (sm * gm).sum(), (st, mt))
    return [ss.detach(), C.detach(), sm.detach(), ds, dm]


def _check_soft_step(out, s, m, gs, gC, gm, T, tag, ctx):
    ss, C, sm, ds, dm = out
    N = s.shape[0]
    ref = _reference(s, m, T, gs, gC, gm)
    _check_forward(ref, C, ss, sm, m, s, N, tag, ctx)
    C64 = C.double()
    _within(dm, C64.t() @ gm.double(), _product_bound(C64.t(), gm.double(), N), f"{tag} d_matrix", ctx)
    _assert_grad_close(ds.cpu().numpy(), ref["d_scores"].cpu().numpy(), f"{tag} d_scores ({ctx})", tol=GRAD_TOL)


def test_vendor_products_from_concurrent_streams(G, backends):
    """Four host threads, each on its own torch stream with operands of its own, enqueue three rounds of: the soft sort forward and backward
    at N = 2048 with a matrix (hipBLASLt: C M, the accumulating dC += g_mat M^T, C^T g_mat), gnms_sgemm at 640 x 2048 x 1024 (rocBLAS) and
    at 2560 x 2048 x 2176 (hipBLASLt), and synchronise only then.  The libraries' handles (and hipBLASLt's workspace) are shared by the
    device's streams.  Every result equals the same call made single-threaded bit for bit (the eager vendor path is deterministic: atomics
    off, one algorithm per shape; checked by running the single-threaded calls twice), and those are checked against float64."""
    from groomed_nms_amd.groomed_nms import _sgemm
    T = 1e-3
    shapes = ((640, 2048, 1024), (2560, 2048, 2176))
    nthreads, rounds = 4, 3
    ops = []
    for t in range(nthreads):
        rng = np.random.default_rng(100 + t)
        N = 2048
        soft = (_uniform_scores(rng, N), _rand(rng, (N, N)), _rand(rng, (N,)), _rand(rng, (N, N)), _rand(rng, (N, N)))
        mats = [(_rand(rng, (M, K)), _rand(rng, (K, Nn))) for M, Nn, K in shapes]
        ops.append((soft, mats))

    def run(t):
        soft, mats = ops[t]
        return _soft_step(G, *soft, T) + [_sgemm(a, b) for a, b in mats]

    refs = [run(t) for t in range(nthreads)]
    again = [run(t) for t in range(nthreads)]
    torch.cuda.synchronize()
    for t in range(nthreads):
        ctx = _ctx(backends, thread=t)
        assert all(torch.equal(x, y) for x, y in zip(refs[t], again[t])), f"single-threaded calls are not reproducible; {ctx}"
        soft, mats = ops[t]
        _check_soft_step(refs[t][:5], *soft, T, f"streams ref t={t}", ctx)
        for (a, b), d, (M, Nn, K) in zip(mats, refs[t][5:], shapes):
            a64, b64 = a.double(), b.double()
            _within(d, a64 @ b64, _product_bound(a64, b64, K), f"streams ref t={t} sgemm {M}x{Nn}x{K}", ctx)
    del again
    results, errors = [None] * nthreads, []

    def worker(t):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                outs = [run(t) for _ in range(rounds)]
                st.synchronize()
            results[t] = outs
        except Exception as e:                                        # noqa: BLE001  (reported below, on the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, f"{errors}; {_ctx(backends)}"
    names = ["soft_scores", "C", "soft_matrix", "d_scores", "d_matrix"] + ["sgemm %dx%dx%d" % sh for sh in shapes]
    bad = [(t, r, names[k]) for t in range(nthreads) for r in range(rounds) for k in range(len(names))
           if not torch.equal(results[t][r][k], refs[t][k])]
    assert not bad, f"results differ from the single-threaded calls: {bad[:8]}; {_ctx(backends)}"


def test_soft_sort_captured_in_a_graph(G, backends):
    """The soft sort forward and backward captured with torch.cuda.graph (one stream, no side branches) at N = 1024 and 2048.  While a
    stream is being captured the vendor libraries refuse and every product runs on the library's own 256 x 128 kernel, unsplit: eagerly
    these sizes split K over partial panels allocated on the stream, and with those panels inside the graph the second replay at N = 1024
    returned a wrong d_matrix.  Two replays on new inputs copied into the static tensors, each checked against float64."""
    T = 1e-3
    for N in (1024, 2048):
        ctx = _ctx(backends, N=N, captured=True)
        rng = np.random.default_rng(N + 7)
        static = [_uniform_scores(rng, N), _rand(rng, (N, N)), _rand(rng, (N,)), _rand(rng, (N, N)), _rand(rng, (N, N))]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                 # warm-up outside the capture
            _soft_step(G, *static, T)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _soft_step(G, *static, T)
        for rep in range(2):
            fresh = [_uniform_scores(rng, N), _rand(rng, (N, N)), _rand(rng, (N,)), _rand(rng, (N, N)), _rand(rng, (N, N))]
            for dst, src in zip(static, fresh):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            _check_soft_step([o.clone() for o in out], *fresh, T, f"graph N={N} replay {rep}", ctx)
        del graph, out
        torch.cuda.empty_cache()
