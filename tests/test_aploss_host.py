"""CPU-side tests of the AP loss (groomed_nms_amd/aploss.py, csrc/aploss.hip): the checker the GPU tests of test_aploss_gpu.py are held to.

`restate` is a plain float64 restatement of the reference's lib/loss/aploss.py:14-78, with its line numbers: the Python loop over the
positives in ascending order, on the float32 inputs widened once.  Here it is
  (a) checked against the reference's own vectors (tests/golden/aploss.npz),
  (b) used to measure e_ref, the distance of the C oracle (oracle.aploss: the reference's fp32 arithmetic in the reference's order) from
      float64, on every case of CASES -- the committed table of shapes, label layouts and logit generators that the GPU file imports,
  (c) mutated in four ways a kernel could plausibly be wrong; every mutant must leave the rule's tolerance by a factor of 16 on every
      case that is not degenerate, so that no GPU comparison against `restate` is vacuous.

The rule: |gpu - restate| <= max(4 e_ref, 4 float32 ulps of the largest entry), for the loss and for the gradient of
each image.  A NaN or infinite logit inside the counted prefix is out of scope: the reference returns NaN there.
"""
import collections
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "aploss.npz")
MUTANTS = ("no_rescale", "a_without_half", "prec_not_running_max", "last_f_mod_4_skipped")
f32 = np.float32


def ulp32(v):
    return float(np.spacing(f32(abs(v))))


def _rank(v, x):
    return np.clip((v - x) / 2.0 + 0.5, 0.0, 1.0)                    # :52-53, :55-56 with delta = 1 (:17)


def restate(logits, targets, tail=0, positive_label=1, negative_label=0, mutant=None):
    """-> (loss, d loss / d logits [n], trips that did not raise max_prec), all float64.  `tail` further negatives of logit 0 behind the
    n boxes, without a gradient of their own (gnms_aploss_tail), in closed form.  `mutant`: one of MUTANTS, for the sensitivity tests."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(logits, f32).astype(np.float64)
    t = np.asarray(targets, f32).astype(np.float64)
    grad = np.zeros(len(x))                                          # :19
    if len(x) == 0 or t.max() <= 0:                                  # :27-29
        return 0.0, grad, 0
    labels_p = t == positive_label                                   # :31
    if not labels_p.any():                                           # (the reference's torch.min raises here; the kernels return 0)
        return 0.0, grad, 0
    fg = x[labels_p]                                                 # :32
    threshold = fg.min() - 1.0                                       # :33
    valid_n = (t == negative_label) & (x >= threshold)               # :36
    bg = x[valid_n]                                                  # :37
    bg_grad = np.zeros(len(bg))                                      # :38
    tail = float(tail) if (tail > 0 and 0.0 >= threshold) else 0.0   # the zero-logit negatives pass :36 or not, all together
    F = len(fg)                                                      # :43
    prec = np.zeros(F)                                               # :44
    order = np.argsort(fg, kind="stable")                            # :47
    if mutant == "last_f_mod_4_skipped" and F >= 2048:
        order = order[:F - F % 4]
    max_prec, stayed = 0.0, 0                                        # :48
    for ii in order:                                                 # :50
        tmp1 = _rank(fg, fg[ii])                                     # :52-53
        tmp2 = _rank(bg, fg[ii])                                     # :55-56
        a = tmp1.sum() + (0.0 if mutant == "a_without_half" else 0.5)   # :58
        b = tmp2.sum() + tail * _rank(0.0, fg[ii])                   # :60
        tmp2 = tmp2 / (a + b)                                        # :61
        current_prec = a / (a + b)                                   # :62
        if max_prec <= current_prec:                                 # :63
            max_prec = current_prec                                  # :64
        else:
            stayed += 1
            if mutant != "no_rescale":
                tmp2 = tmp2 * ((1.0 - max_prec) / (1.0 - current_prec))   # :66
        bg_grad += tmp2                                              # :67
        prec[ii] = current_prec if mutant == "prec_not_running_max" else max_prec   # :68
    grad[valid_n] = bg_grad                                          # :70
    grad[labels_p] = -(1.0 - prec)                                   # :71
    grad /= max(F, 1)                                                # :73, :75
    return 1.0 - prec.sum() / max(F, 1), grad, stayed                # :78, :80


def restate_explicit_tail(logits, targets, tail, positive_label=1, negative_label=0):
    """the same with the tail written out as `tail` boxes of logit 0 and the negative label; their gradient is dropped"""
    n, k = len(logits), max(int(tail), 0)
    loss, grad, stayed = restate(np.concatenate([np.asarray(logits, f32), np.zeros(k, f32)]),
                                 np.concatenate([np.asarray(targets, f32), np.full(k, negative_label, f32)]), 0, positive_label, negative_label)
    return loss, grad[:n], stayed


def valid_negatives(logits, targets, positive_label=1, negative_label=0):
    """G, the number of negatives at or above the smallest positive - 1 (:33, :36)"""
    x, t = np.asarray(logits, f32), np.asarray(targets, f32)
    return int(((t == negative_label) & (x >= x[t == positive_label].min() - f32(1.0))).sum())


# ------------------------------------------------------------------------------------------------ the case table
# One row per launch.  `F`, `counts` and `tail` are per DISTINCT image; B > len(F) repeats the distinct images in turn (image b is
# distinct image b % len(F)).  counts None: every image has N boxes.  tail None: gnms_aploss (ap_loss_batched); a tuple: gnms_aploss_tail.
# Every image has 5 % of its boxes labelled -1 (ignored) where negatives are left for it, and every batch of three or more has one image
# without a positive (F = 0).  The route each row takes is asserted in test_aploss_gpu.py next to a restatement of aploss_impl's dispatch.
Case = collections.namedtuple("Case", "name B N counts F tail gen seed")

DEGENERATE = ("equal",)          # every trip has the same precision: no rescale, nothing for three of the mutants to change


def _lds1(N, gen, seed):
    return [Case("lds1_n%d" % N, 3, N, (N, N - 5, N // 2), (1, N // 2, 0), None, gen, seed),
            Case("lds1_n%d_all" % N, 3, N, (N, N, N // 2), (2, N, 0), None, "equal", seed + 1)]          # F = N: no negative at all


def _tail(N, E, F, gen, seed):
    return Case("tail_n%d_e%d" % (N, E), 4, N, (N, N - 5, (3 * N) // 4, N), F, (0, E, E - 3, 5), gen, seed)


CASES = [
    # aploss_kernel<1>: N <= 1024
    Case("lds1_n1", 1, 1, None, (1,), None, "normal1", 1),
    Case("lds1_n2", 2, 2, None, (1, 2), None, "normal1", 2),
    *_lds1(63, "normal05", 3), *_lds1(64, "ties8", 5), *_lds1(65, "normal2", 7), *_lds1(1024, "normal1", 9),
    Case("lds1_zero", 3, 1024, (1024, 1019, 512), (300, 64, 0), None, "signed_zero", 11),
    Case("lds1_nonmonotone", 3, 1024, (1024, 1019, 512), (300, 64, 0), None, "nonmonotone", 12),
    Case("lds1_separated", 3, 1024, (1024, 1019, 512), (300, 64, 0), None, "separated_top", 713),
    # aploss_kernel<2>: 1024 < N < 2048, and N = 2048 with B > 64
    Case("lds2_n1025", 3, 1025, (1025, 1020, 512), (200, 512, 0), None, "normal1", 14),
    Case("lds2_n2047", 3, 2047, (2047, 2042, 1023), (1023, 100, 0), None, "normal2", 15),
    Case("lds2_b65_n2048", 65, 2048, (2048, 2043, 1024), (64, 9, 0), None, "normal1", 116),
    # aploss_kernel<4> through gnms_aploss: 2048 < N <= 4096 with B > 64
    Case("lds4_b65_n2049", 65, 2049, (2049, 2044, 1024), (64, 9, 0), None, "ties8", 717),
    Case("lds4_b65_n4096", 65, 4096, (4096, 4091, 2048), (64, 33, 0), None, "normal1", 18),
    # aploss_kernel<4> through gnms_aploss_tail: 2048 < N <= 4096, whatever B is (B = 4 here: three F and the image without positives)
    _tail(2049, 1, (1, 300, 1025, 0), "normal1", 119), _tail(2049, 700, (1025, 1, 300, 0), "normal05", 120),
    _tail(2500, 1, (300, 1025, 1, 0), "ties8", 21), _tail(2500, 700, (1, 300, 1025, 0), "signed_zero", 22),
    _tail(4096, 1, (1025, 1, 300, 0), "nonmonotone", 23), _tail(4096, 700, (300, 1025, 1, 0), "normal2", 24),
    Case("tail_outside", 2, 2049, (2049, 2044), (300, 64), (700, 5), "positives_above_one", 25),
    # the spread kernels: N >= 2048 with B <= 64, N > 4096.  ap_prepare_kernel<2, 4, 8, 16>, its sort tiers, ap_rank_body<1 or 4>
    Case("spread_n2048", 3, 2048, (2048, 2043, 1024), (1024, 1, 0), None, "normal2", 26),
    Case("spread_n2048_zero", 3, 2048, (2048, 2043, 1024), (500, 40, 0), None, "signed_zero", 27),
    Case("spread_n2048_all", 3, 2048, (2048, 2043, 1024), (100, 2043, 0), None, "equal", 28),
    Case("spread_n2049", 3, 2049, (2049, 2044, 1024), (700, 64, 0), None, "ties8", 29),
    Case("spread_n4097_a", 3, 4097, (4097, 4092, 2048), (1025, 2047, 0), None, "normal1", 30),
    Case("spread_n4097_b", 3, 4097, (4097, 4092, 2048), (2048, 300, 0), None, "separated_top", 31),
    Case("spread_n8193_a", 3, 8193, (8193, 8188, 4096), (2049, 2051, 0), None, "normal05", 32),
    Case("spread_n8193_b", 3, 8193, (8193, 8188, 4096), (4096, 2050, 0), None, "nonmonotone", 33),
    Case("spread_n16384_a", 3, 16384, (16384, 16379, 8192), (8192, 4097, 0), None, "normal1", 34),
    Case("spread_n16384_b", 3, 16384, (16384, 16379, 8192), (8195, 2, 0), None, "normal1", 35),
    # the rank loop's chunks of 64 * 32 values: G = 2047, 2048, 2049 valid negatives beside F = 2049 (B = 4: three G and the empty image)
    Case("spread_chunks", 4, 4400, (2049 + 2047 + 215, 2049 + 2048 + 215, 2049 + 2049 + 215, 2200), (2049, 2049, 2049, 0), None, "all_valid", 36),
]
CASE_NAMES = [c.name for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES)
CHUNK_G = (2047, 2048, 2049)


def case_of(name):
    return CASES[CASE_NAMES.index(name)]


def distinct(c):
    return len(c.F)


def count_of(c, i):
    return c.N if c.counts is None else c.counts[i]


@functools.lru_cache(maxsize=None)
def _image(name, i):
    c = case_of(name)
    n, F = count_of(c, i), c.F[i]
    rng = np.random.default_rng([c.seed, i])
    ignored = min(n - F, int(round(0.05 * n)))
    if c.gen == "all_valid":
        ignored = n - F - CHUNK_G[i] if F else ignored
    perm = rng.permutation(n)
    t = np.zeros(n, f32)
    t[perm[:F]] = 1
    t[perm[F:F + ignored]] = -1
    pos, neg = t == 1, t == 0
    sigma = {"normal05": 0.5, "normal2": 2.0}.get(c.gen, 1.0)
    x = rng.normal(0.0, sigma, n)
    if c.gen == "ties8":                                             # ties among positives, among negatives and between them
        x = np.round(x * 8) / 8
    elif c.gen == "equal":
        x[:] = 0.25
    elif c.gen == "signed_zero":                                     # half of the positives and a tenth of the negatives are +0.0 or -0.0
        z = np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0)
        pick = (pos & (rng.uniform(size=n) < 0.5)) | (neg & (rng.uniform(size=n) < 0.1))
        x = np.where(pick, z, x)
    elif c.gen == "nonmonotone":                                     # positives, then a block of negatives, then positives: while the
        k = np.flatnonzero(pos)                                      # trips walk up the lower block the precision falls
        x[neg] = rng.normal(0.0, 0.6, int(neg.sum()))
        x[k[:len(k) // 2]] = rng.normal(-2.5, 0.4, len(k) // 2)
        x[k[len(k) // 2:]] = rng.normal(1.5, 0.8, len(k) - len(k) // 2)
    elif c.gen == "separated_top" and F:                             # the upper quarter of the positives more than 1 above every negative
        k = np.flatnonzero(pos)
        top = k[np.argsort(x[k])[len(k) - max(len(k) // 4, 1):]]
        x[top] += max(x[neg].max() + 1.25 - x[top].min(), 0.0) if neg.any() else 0.0
    elif c.gen == "positives_above_one":                             # the smallest positive above 1: zero-logit negatives are outside the window
        x[pos] = 1.0625 + 1.5 * np.abs(x[pos])
        x[neg] = 2.0 + 1.5 * x[neg]
    elif c.gen == "all_valid" and F:                                 # every negative inside the window: G is what the table says
        x[neg] = np.maximum(x[neg], x[pos].min() - 0.75)
    x = x.astype(f32)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def image(name, i):
    """(logits [n], targets [n]) float32 of distinct image i of the case, n = its count; read-only, shared"""
    return _image(name, i)


def tail_of(c, i):
    return 0 if c.tail is None else c.tail[i]


@functools.lru_cache(maxsize=None)
def restated(name, mutant=None):
    """per distinct image: (loss, grad [n], trips that did not raise max_prec)"""
    c = case_of(name)
    out = []
    for i in range(distinct(c)):
        loss, grad, stayed = restate(*image(name, i), tail=tail_of(c, i), mutant=mutant)
        grad.setflags(write=False)
        out.append((loss, grad, stayed))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_errors(name):
    """e_ref per distinct image: (|loss|, largest |gradient entry|) of oracle - restate; the tail goes to the oracle written out"""
    c = case_of(name)
    out = []
    for i, (loss, grad, _) in enumerate(restated(name)):
        x, t = image(name, i)
        k = max(tail_of(c, i), 0)
        ol, og = O.aploss(np.concatenate([x, np.zeros(k, f32)]), np.concatenate([t, np.zeros(k, f32)]))
        out.append((abs(ol - loss), float(np.abs(og[:len(x)].astype(np.float64) - grad).max()) if len(x) else 0.0))
    return tuple(out)


def tolerances(name):
    """the rule, per distinct image: (loss, gradient)"""
    return tuple((max(4 * el, 4 * ulp32(loss)), max(4 * eg, 4 * ulp32(np.abs(grad).max())))
                 for (loss, grad, _), (el, eg) in zip(restated(name), oracle_errors(name)))


def is_degenerate(c, i):
    return c.gen in DEGENERATE or c.F[i] < 8


# ------------------------------------------------------------------------------------------------ (a) the reference's vectors
def test_restatement_reproduces_the_reference_vectors():
    """e_ref of the reference itself (torch's fp32 sums): at most 4 ulps of the loss and 64 ulps of the largest gradient entry, the
    caps of the oracle below; an image without a positive and one without a negative are exact"""
    z = np.load(GOLDEN)
    tags = sorted({k.split("/")[0] for k in z.keys()})
    assert len(tags) >= 12
    for tag in tags:
        x, t, up = z[tag + "/logits"], z[tag + "/targets"], float(z[tag + "/upstream"])
        loss, grad, stayed = restate(x, t)
        e_loss = abs(float(z[tag + "/loss"].reshape(-1)[0]) - loss)
        e_grad = float(np.abs(z[tag + "/grad"].astype(np.float64) - grad * up).max())
        F = int((t == 1).sum())
        top = float(np.abs(grad * up).max())
        if tag == "u500_499":        # 499 positives of 500 boxes: loss 0.002 = 1 - 0.998 (:80) and gradients -(1 - prec) / F (:71) are differences
            assert loss < 0.01       # of fp32 numbers next to 1, so the reference's error is in ulps of 1 and of 1 / F, not of the result
            loss_scale, top_scale, cap = 1.0, top / loss, 4          # (and the rescale factor of :66 is a quotient of two of them:
        else:                                                        # its relative error is an ulp of 1 over 1 - prec, about the loss)
            loss_scale, top_scale, cap = loss, top, 64
        print("%-10s F %4d stayed %4d  e_ref: loss %.3g (%.2f ulps of %.3g)  gradient %.3g (%.2f ulps of %.3g)"
              % (tag, F, stayed, e_loss, e_loss / ulp32(loss_scale) if loss else 0.0, loss_scale, e_grad,
                 e_grad / ulp32(top_scale) if top else 0.0, top_scale))
        assert e_loss <= 4 * ulp32(loss_scale), tag
        assert e_grad <= cap * ulp32(top_scale), tag
        if tag in ("nopos", "allpos"):
            assert loss == 0.0 and not grad.any()


# ------------------------------------------------------------------------------------------------ the table itself
def test_the_table_is_what_it_says():
    for c in CASES:
        D = distinct(c)
        assert c.B >= D and (c.counts is None or len(c.counts) == D) and (c.tail is None or len(c.tail) == D), c.name
        assert D < 3 or 0 in c.F, c.name                                        # an image without positives in every batch of three or more
        for i in range(D):
            x, t = image(c.name, i)
            n = count_of(c, i)
            assert len(x) == len(t) == n <= c.N and int((t == 1).sum()) == c.F[i] and np.isfinite(x).all(), (c.name, i)
            assert int((t == -1).sum()) == int(round(0.05 * n)) or c.F[i] + int((t == -1).sum()) == n or c.gen == "all_valid", (c.name, i)
    for i, G in enumerate(CHUNK_G):
        assert valid_negatives(*image("spread_chunks", i)) == G
    for name in ("lds1_separated", "spread_n4097_b"):                           # prec is 1 on the upper quarter
        for i in (0, 1):
            x, t = image(name, i)
            top = np.sort(x[t == 1])[-(int((t == 1).sum()) // 4):]
            assert top.min() > x[t == 0].max() + 1.0
    for i in (0, 1):
        x, t = image("tail_outside", i)
        assert x[t == 1].min() > 1.0
    x, t = image("lds1_zero", 0)
    assert np.signbit(x[(t == 1) & (x == 0)]).any() and not np.signbit(x[(t == 1) & (x == 0)]).all()


def test_non_monotone_cases_keep_a_quarter_of_the_trips_from_rising():
    for c in CASES:
        if c.gen == "nonmonotone":
            for i, (_, _, stayed) in enumerate(restated(c.name)):
                if c.F[i] >= 8:
                    print("%s image %d: %d of %d trips do not raise max_prec" % (c.name, i, stayed, c.F[i]))
                    assert 4 * stayed >= c.F[i], (c.name, i)


def test_closed_form_tail_is_the_explicit_tail():
    """tail * clamp((0 - x) / 2 + 0.5, 0, 1) added to b when 0 >= min positive - 1, against zero-logit negatives written out: 1e-13"""
    seen = 0
    for c in CASES:
        if c.tail is None:
            continue
        for i, (loss, grad, stayed) in enumerate(restated(c.name)):
            el, eg, es = restate_explicit_tail(*image(c.name, i), c.tail[i])
            assert abs(el - loss) <= 1e-13 and (np.abs(eg - grad).max() if len(grad) else 0.0) <= 1e-13 and es == stayed, (c.name, i)
            seen += c.tail[i] > 0 and c.F[i] > 0
    assert seen >= 11
    c = case_of("tail_outside")
    for i in range(2):                                                          # outside the window: as if there were none
        a, b = restated(c.name)[i], restate(*image(c.name, i), tail=0)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ (b) the oracle's own error
@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_error_is_small(name):
    """e_ref <= 4 ulps of the loss and 64 ulps of the largest gradient entry (a sequential fp32 sum of F terms: ~sqrt(F) typical)"""
    c = case_of(name)
    for i, ((loss, grad, stayed), (el, eg)) in enumerate(zip(restated(name), oracle_errors(name))):
        top = float(np.abs(grad).max()) if len(grad) else 0.0
        print("%-18s image %d n %5d F %4d stayed %4d  e_ref: loss %.3g (%.2f ulps)  gradient %.3g (%.2f ulps of %.3g)"
              % (name, i, count_of(c, i), c.F[i], stayed, el, el / ulp32(loss) if loss else 0.0, eg, eg / ulp32(top) if top else 0.0, top))
        assert el <= 4 * ulp32(loss), (name, i)
        assert eg <= 64 * ulp32(top), (name, i)
        if c.F[i] == 0:
            assert loss == 0.0 and top == 0.0


# ------------------------------------------------------------------------------------------------ (c) sensitivity
def margin(name, i, mutant):
    """how far the mutant is from the restatement, in units of the rule's tolerance: the larger of loss and gradient"""
    (loss, grad, _), (ml, mg, _), (tl, tg) = restated(name)[i], restated(name, mutant)[i], tolerances(name)[i]
    return max(abs(ml - loss) / tl, float(np.abs(mg - grad).max()) / tg)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_mutants_leave_the_tolerance(name):
    c = case_of(name)
    for i in range(distinct(c)):
        if c.F[i] == 0:
            continue
        for m in MUTANTS:
            applies = c.F[i] >= 2048 and c.F[i] % 4 != 0 if m == "last_f_mod_4_skipped" else not is_degenerate(c, i)
            if not applies:
                continue
            r = margin(name, i, m)
            print("%-18s image %d F %4d %-22s %.0f x tolerance" % (name, i, c.F[i], m, r))
            assert r >= 16, (name, i, m, r)


def test_the_fourth_mutant_has_cases():
    hit = [(c.name, F) for c in CASES for F in c.F if F >= 2048 and F % 4]
    assert {F % 4 for _, F in hit} == {1, 2, 3} and len(hit) >= 6
