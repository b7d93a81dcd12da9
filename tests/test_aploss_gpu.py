"""GPU tests of the AP loss (groomed_nms_amd/aploss.py, csrc/aploss.hip) against the float64 restatement of tests/test_aploss_host.py, on
every kernel route, over the case table that file commits.

The rule: |gpu - restate| <= max(4 e_ref, 4 float32 ulps of the largest entry), for the loss and, per image, for the
gradient; e_ref = |C oracle - restate| on the same image (test_aploss_host.oracle_errors).  Exact, always: the gradient is 0 at ignored
labels, at and past counts[b] (where these tests put NaN logits with the positive label) and in an image without positives, whose loss
is 0; a repeated image gives the bits of its original.  Each test prints |gpu - restate| / tolerance before it asserts; the figures per
route are in DESIGN.md 3.17.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_aploss_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def route_of(B, N, tail):
    """aploss_impl's dispatch (csrc/aploss.hip), restated: which shape selects which kernel.
         spread<E>  ap_prepare_kernel<E> + ap_rank_kernel + ap_scan_kernel<E> + ap_neg_grad_kernel, E = (next power of two >= max(N, 1024)) / 1024:
                    `!tail_counts && (N > kApMaxN || (N >= 2048 && B <= 64))`, kApMaxN = 4096
         lds<E>     aploss_kernel<E>, one workgroup per image: E = 1 for N <= 1024, 2 for N <= 2048, 4 for N <= 4096 (96 KiB of dynamic LDS)"""
    if not tail and (N > 4096 or (N >= 2048 and B <= 64)):
        P2 = 1024
        while P2 < N:
            P2 <<= 1
        return "spread%d" % (P2 // 1024)
    assert N <= 4096
    return "lds1" if N <= 1024 else ("lds2" if N <= 2048 else "lds4")


def sort_tier(E, F):
    """ap_prepare_kernel<E> sorts the smallest of 1024, 2048, 4096, 8192 slots that holds the F keys (GNMS_AP_SORT), all 1024 E slots otherwise"""
    for EE in (1, 2, 4, 8):
        if E > EE and F <= 1024 * EE:
            return EE
    return E


# the route every row of the table is there for; test_every_case_takes_its_route holds the table to it
ROUTES = dict(
    lds1="lds1_n1 lds1_n2 lds1_n63 lds1_n63_all lds1_n64 lds1_n64_all lds1_n65 lds1_n65_all lds1_n1024 lds1_n1024_all lds1_zero lds1_nonmonotone "
         "lds1_separated",
    lds2="lds2_n1025 lds2_n2047 lds2_b65_n2048",
    lds4="lds4_b65_n2049 lds4_b65_n4096 tail_n2049_e1 tail_n2049_e700 tail_n2500_e1 tail_n2500_e700 tail_n4096_e1 tail_n4096_e700 tail_outside",
    spread2="spread_n2048 spread_n2048_zero spread_n2048_all",
    spread4="spread_n2049",
    spread8="spread_n4097_a spread_n4097_b spread_chunks",
    spread16="spread_n8193_a spread_n8193_b spread_n16384_a spread_n16384_b",
)


def test_every_case_takes_its_route():
    named = {n: r for r, names in ROUTES.items() for n in names.split()}
    assert sorted(named) == sorted(H.CASE_NAMES)
    for c in H.CASES:
        assert route_of(c.B, c.N, c.tail is not None) == named[c.name], c.name
    # the sort tiers of ap_prepare_kernel and both bodies of ap_rank_kernel (F >= 2048: four positives per wave)
    tiers = {(int(named[c.name][6:]), sort_tier(int(named[c.name][6:]), F)) for c in H.CASES if named[c.name].startswith("spread") for F in c.F if F}
    assert {(2, 1), (4, 1), (8, 1), (8, 2), (16, 4), (16, 8), (16, 16)} <= tiers
    spread_F = {F for c in H.CASES if named[c.name].startswith("spread") for F in c.F}
    assert {1, 1024, 1025, 2047, 2048, 2049, 2051, 4096, 4097, 8192, 8195} <= spread_F
    assert {F % 4 for F in spread_F if F >= 2048} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def dev():
    from groomed_nms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def batch(c, width=None):
    """-> logits [B][width] (NaN from counts[b] on), targets [B][width] (the positive label from counts[b] on), counts [B] or None, tails [B] or None"""
    W, D = width or c.N, H.distinct(c)
    lg, tg = np.full((c.B, W), np.nan, f32), np.ones((c.B, W), f32)
    for b in range(c.B):
        x, t = H.image(c.name, b % D)
        lg[b, :len(x)], tg[b, :len(x)] = x, t
    counts = None if (c.counts is None and W == c.N) else np.array([H.count_of(c, b % D) for b in range(c.B)], np.int32)
    tails = None if c.tail is None else np.array([c.tail[b % D] for b in range(c.B)], np.int32)
    return lg, tg, counts, tails


def run_batched(dev, lg, tg, counts, weights=None, active=None):
    """ap_loss_batched and its backward -> loss [B], d (sum_b w_b loss_b) / d logits [B][N] as NumPy"""
    from groomed_nms_amd.aploss import ap_loss_batched
    lt = _t(lg, dev).requires_grad_(True)
    loss = ap_loss_batched(lt, _t(tg, dev), active=None if active is None else _t(active, dev), counts=None if counts is None else _t(counts, dev))
    (loss.sum() if weights is None else (loss * _t(np.asarray(weights, f32), dev)).sum()).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy(), lt.grad.cpu().numpy()


def run_tail(dev, lg, tg, counts, tails):
    """gnms_aploss_tail as groomed_nms_amd/after_nms.py calls it; the outputs start as NaN"""
    from groomed_nms_amd import _lib
    lib = _lib.load()
    B, N = lg.shape
    a, b, c, d = _t(lg, dev), _t(tg, dev), None if counts is None else _t(counts, dev), _t(tails, dev)
    loss, grad = torch.full((B,), np.nan, device=dev), torch.full((B, N), np.nan, device=dev)
    _lib.check(lib.gnms_aploss_tail(_lib.ptr(a), _lib.ptr(b), B, N, _lib.ptr(c), _lib.ptr(d), 1.0, 0.0, _lib.ptr(loss), _lib.ptr(grad),
                                    _lib.stream_ptr()), "gnms_aploss_tail")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy()


def run_case(dev, c, width=None):
    lg, tg, counts, tails = batch(c, width)
    return run_tail(dev, lg, tg, counts, tails) if tails is not None else run_batched(dev, lg, tg, counts)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.int32), np.ascontiguousarray(b, f32).view(np.int32))


def check(c, loss, grad, what=None, bound=None):
    """the rule on every distinct image, the exact properties on every image.  bound: (loss, gradient) tolerances of a route that has its
    own, per distinct image, in place of the rule's"""
    what = what or c.name
    D = H.distinct(c)
    want, tol = H.restated(c.name), bound or H.tolerances(c.name)
    rl, rg = 0.0, 0.0
    for b in range(c.B):
        n = H.count_of(c, b % D)
        assert not grad[b, n:].any(), "%s image %d: gradient past its count" % (what, b)
        if b >= D:
            assert same_bits(loss[b], loss[b % D]) and same_bits(grad[b], grad[b % D]), "%s: image %d differs from image %d" % (what, b, b % D)
            continue
        wl, wg, _ = want[b]
        t = H.image(c.name, b)[1]
        assert np.isfinite(loss[b]) and np.isfinite(grad[b]).all(), (what, b)
        assert not grad[b, :n][t == -1].any(), "%s image %d: gradient at an ignored label" % (what, b)
        assert not grad[b, :n][wg == 0].any(), "%s image %d: gradient where the restatement has exactly 0" % (what, b)
        if c.F[b] == 0:
            assert loss[b] == 0.0 and not grad[b].any(), "%s image %d has no positive" % (what, b)
            continue
        dl, dg = abs(float(loss[b]) - wl), float(np.abs(grad[b, :n].astype(np.float64) - wg).max())
        rl, rg = max(rl, dl / tol[b][0]), max(rg, dg / tol[b][1])
        print("%s image %d (n %d, F %d): |gpu - restate| / tolerance: loss %.3f (%.3g / %.3g) gradient %.3f (%.3g / %.3g)"
              % (what, b, n, c.F[b], dl / tol[b][0], dl, tol[b][0], dg / tol[b][1], dg, tol[b][1]))
    print("%s: |gpu - restate| / tolerance: loss %.3f gradient %.3f" % (what, rl, rg))
    assert rl <= 1.0 and rg <= 1.0, (what, rl, rg)
    return rl, rg


@pytest.mark.parametrize("name", H.CASE_NAMES)
def test_case_against_restatement(dev, name):
    c = H.case_of(name)
    loss, grad = run_case(dev, c)
    check(c, loss, grad)


def test_lds_route_and_spread_route_on_the_same_images(dev):
    """N = 2047: aploss_kernel<2>.  The same boxes in rows of 2048 with their counts: the spread kernels.  Each within the rule of restate"""
    c = H.case_of("lds2_n2047")
    assert route_of(c.B, 2047, False) == "lds2" and route_of(c.B, 2048, False) == "spread2"
    check(c, *run_case(dev, c), what="lds2_n2047 (LDS)")
    loss, grad = run_case(dev, c, width=2048)
    assert grad.shape == (3, 2048)
    check(c, loss, grad, what="lds2_n2047 in rows of 2048 (spread)")


def test_tail_outside_the_window_is_no_tail(dev):
    """the smallest positive is above 1: zero-logit negatives fail `logit >= min positive - 1`, and the result has the bits of tail 0"""
    c = H.case_of("tail_outside")
    lg, tg, counts, tails = batch(c)
    assert (tails > 0).all()
    with_tail, without = run_tail(dev, lg, tg, counts, tails), run_tail(dev, lg, tg, counts, np.zeros_like(tails))
    assert same_bits(with_tail[0], without[0]) and same_bits(with_tail[1], without[1])
    neg = run_tail(dev, lg, tg, counts, -tails)
    assert same_bits(neg[0], without[0]) and same_bits(neg[1], without[1])


@pytest.mark.parametrize("name", ["lds2_n1025", "spread_n2049", "lds4_b65_n2049"])
def test_upstream_weights_scale_the_stored_gradient(dev, name):
    c = H.case_of(name)
    lg, tg, counts, _ = batch(c)
    w = np.array([(1.5, 3.0, 0.7)[b % 3] * (1 + b // 3) for b in range(c.B)], f32)
    l1, g1 = run_batched(dev, lg, tg, counts)
    lw, gw = run_batched(dev, lg, tg, counts, weights=w)
    assert same_bits(l1, lw) and same_bits(gw, g1 * w[:, None])


CHILD_CASES = ("lds2_n1025", "spread_n2049")
_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, "tests")
from groomed_nms_amd import groomed_nms as GN
import test_aploss_gpu as T
assert not GN._binding()
dev = torch.device("cuda", 0)
out = {}
for name in T.CHILD_CASES:
    lg, tg, counts, _ = T.batch(T.H.case_of(name))
    out[name + "/loss"], out[name + "/grad"] = T.run_batched(dev, lg, tg, counts, weights=T.child_weights(len(lg)))
np.savez(sys.argv[1], **out)
"""


def child_weights(B):
    return np.linspace(0.5, 2.0, B).astype(f32)


def test_both_bindings_give_the_same_bits(dev):
    """ap_loss_batched through the C++ autograd node (this process) and through _APLossBatched on the ctypes path (a fresh child process)"""
    from groomed_nms_amd import groomed_nms as GN
    assert GN._binding(), "the C++ binding is not in use in this process"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ctypes.npz")
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _CHILD, path], cwd=root, env=dict(os.environ, GNMS_BINDING="ctypes"),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        child = np.load(path)
        for name in CHILD_CASES:
            lg, tg, counts, _ = batch(H.case_of(name))
            loss, grad = run_batched(dev, lg, tg, counts, weights=child_weights(len(lg)))
            assert same_bits(loss, child[name + "/loss"]) and same_bits(grad, child[name + "/grad"]), name


@pytest.mark.parametrize("name", ["lds2_n1025", "spread_n2049"])
def test_active_mask_is_the_ignored_label(dev, name):
    c = H.case_of(name)
    lg, tg, counts, _ = batch(c)
    active = np.random.default_rng(41).uniform(size=lg.shape) < 0.8
    masked = run_batched(dev, lg, tg, counts, active=active)
    relabelled = run_batched(dev, lg, np.where(active, tg, f32(-1)), counts)
    assert same_bits(masked[0], relabelled[0]) and same_bits(masked[1], relabelled[1])
    assert not masked[1][~active].any() and masked[1].any()
    plain = run_batched(dev, lg, tg, counts)
    assert not same_bits(masked[1], plain[1])


@pytest.mark.parametrize("name", ["lds2_n1025", "spread_n2049"])
def test_other_labels_give_the_same_bits(dev, name):
    """positive_label 2, negative_label 1, everything else ignored (:31, :36): the bits of labels 1 / 0 / -1"""
    from groomed_nms_amd.aploss import ap_loss_batched
    c = H.case_of(name)
    lg, tg, counts, _ = batch(c)
    want = run_batched(dev, lg, tg, counts)
    lt = _t(lg, dev).requires_grad_(True)
    loss = ap_loss_batched(lt, _t(tg + 1, dev), counts=_t(counts, dev), positive_label=2, negative_label=1)
    loss.sum().backward()
    assert same_bits(loss.detach().cpu().numpy(), want[0]) and same_bits(lt.grad.cpu().numpy(), want[1])


@pytest.mark.parametrize("name", ["lds2_n2047", "spread_n4097_a"])
def test_second_call_from_a_side_stream_gives_the_same_bits(dev, name):
    c = H.case_of(name)
    lg, tg, counts, _ = batch(c)
    first = run_batched(dev, lg, tg, counts)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        second = run_batched(dev, lg, tg, counts)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])


def test_argument_checks_return_their_codes(dev):
    from groomed_nms_amd import _lib
    from groomed_nms_amd.aploss import ap_loss_batched
    lib = _lib.load()
    z = torch.zeros((1, 4097), device=dev)
    out, tail = torch.zeros((1,), device=dev), torch.ones((1,), dtype=torch.int32, device=dev)
    args = (_lib.ptr(z), _lib.ptr(z), 1, 4097, None)
    assert lib.gnms_aploss_tail(*args, _lib.ptr(tail), 1.0, 0.0, _lib.ptr(out), _lib.ptr(z), _lib.stream_ptr()) == -2     # GNMS_ERR_UNSUPPORTED
    assert b"4096" in lib.gnms_last_error()
    assert lib.gnms_aploss_tail(*args[:3], 4096, None, None, 1.0, 0.0, _lib.ptr(out), _lib.ptr(z), _lib.stream_ptr()) == -1   # INVALID_ARGUMENT
    assert lib.gnms_aploss(*args[:2], 1, 16385, None, 1.0, 0.0, _lib.ptr(out), _lib.ptr(z), _lib.stream_ptr()) == -2
    with pytest.raises(ValueError):
        ap_loss_batched(z, z[:, :5])
    torch.cuda.synchronize()
