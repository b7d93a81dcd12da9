"""The masked-group backward from the plan the forward leaves behind (bwd_plan_kernel, csrc/nms_backward_kernels.h).

Every builder of the groups' runs (csr_build_body beside the fast tail and in the one launch, groups_body = K5 proper) also writes one plan entry
per position: the members run after run, then the ranks in no group, then the padding.  The backward reads an entry, then pre / plead /
dL/dprob of its rank, and stores; a head sums its members' products from the workgroup's LDS tile (256 positions + a halo of 128), a run longer
than the halo is walked by a whole wave.  Every case here goes through the C ABI, one forward + backward, and compares per image with the CPU
oracle: grad_scores bit for bit, prob bit for bit, the two index lists.  The same cases run once more in a fresh child process with
GNMS_BWD_PLAN=0 (bwd_masked_fused_kernel, the backward that walks hlist / gstart / glen / gsorted): the two kernels' grad_scores must have
the same BITS, signs of zeros included.

Built images (`built`): clusters of near-identical boxes far from each other, so that the groups are the clusters, and leader scores that
fall from cluster to cluster, so that the runs lie in the plan in the order the sizes are listed -- the positions of the runs are chosen,
not found.  Scores span (-0.3, 1.3): heads and members on both sides of the clamp.  dL/dprob ~ N(0, 1) with exact zeros and -0.0.
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from test_grad_iou_host import DEFAULTS, asymmetric

pytestmark = pytest.mark.gpu

HALO = 128                     # kPlanHalo
# run sizes, default group_size = 100 (cap 101), no cluster above the cap: [0,60) [60,70) straddles 64; [70,128) ends on 128; [128,229) a run
# of exactly the cap that starts on a boundary; [229,269) straddles 256; [269,368); [368,384) ends on 384; then runs of 9, 10 and 11 (the
# per-lane sum takes 8 members, the wave the rest), 2, 3 and singletons between them
GEOMETRY = [60, 10, 58, 101, 40, 99, 16, 9, 1, 10, 2, 11, 1, 1, 3, 65, 64, 2]


def built(seed, n, sizes):
    """boxes [n,4], scores [n], dL/dprob [n]: clusters of the given sizes in plan order, the rest singletons; shuffled"""
    rng = np.random.default_rng(seed)
    sizes = list(sizes) + [1] * (n - sum(sizes))
    assert sum(sizes) == n
    C = len(sizes)
    boxes, scores = [], []
    for c, m in enumerate(sizes):
        lead = 1.3 - 1.6 * c / max(C - 1, 1)                            # leader scores fall with the cluster: 1.3 ... -0.3
        x0, y0 = 300.0 * (c % 64), 300.0 * (c // 64)
        jit = rng.uniform(-3, 3, size=(m, 4))
        boxes.append(np.array([x0, y0, x0 + 100, y0 + 100]) + jit)      # IoU inside a cluster >= 0.78, across clusters 0
        s = lead - rng.uniform(0.05, 0.7, size=m)
        s[0] = lead
        scores.append(s)
    boxes, scores = np.concatenate(boxes).astype(np.float32), np.concatenate(scores).astype(np.float32)
    scores += (np.arange(n) * 1e-6).astype(np.float32)                  # tie-free
    assert len(np.unique(scores)) == n
    gp = rng.normal(0, 1, size=n).astype(np.float32)
    gp[rng.random(n) < 0.1] = 0.0
    gp[rng.random(n) < 0.1] = -0.0
    p = rng.permutation(n)
    return boxes[p], scores[p], gp[p]


def random_2d(seed, n, per):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    gp = rng.normal(0, 1, size=n).astype(np.float32)
    gp[::7] = 0.0
    gp[3::11] = -0.0
    return synthetic.clustered_boxes_2d(rng, n, per), synthetic.tie_free_scores(rng, n, -0.3, 1.3), gp


def random_3d(seed, n, per):
    from groomed_nms_amd import synthetic
    rng = np.random.default_rng(seed)
    gp = rng.normal(0, 1, size=n).astype(np.float32)
    gp[::5] = -0.0
    return synthetic.boxes_3d(rng, n, True, per), synthetic.tie_free_scores(rng, n, -0.3, 1.3), gp


def _stack(images):
    return tuple(np.stack([im[i] for im in images]) for i in range(3))


# tag -> (entry, images = (src [B,N,4|7], scores [B,N], dL/dprob [B,N]), counts, keywords, asym)
#   entries: "matrix" gnms_iou2d + gnms_forward, "one2d" gnms_forward_with_iou2d, "one3d" gnms_forward_with_iou3d
@functools.lru_cache(maxsize=1)
def cases():
    c = {}
    geo = lambda n, seed=1: _stack([built(seed, n, GEOMETRY)])
    # forward routes (LABNOTES R12.2 / R14): the one launch from boxes and matrix-in; tail_kernel with the fast tail; the general scan behind an
    # asymmetric matrix; the from-boxes writer launch 2D and 3D (1024 < N <= 4096); the separate tail above 4096
    c["geo one-launch boxes"] = ("one2d", geo(1000), [1000], {}, False)
    c["geo one-launch matrix"] = ("matrix", geo(1000), [1000], {}, False)
    c["geo tail_kernel"] = ("matrix", geo(1088), [1088], {}, False)
    c["geo general scan"] = ("matrix", geo(1088), [1088], {}, True)
    c["geo writer launch 2D"] = ("one2d", geo(1088), [1088], {}, False)
    c["random writer launch 3D"] = ("one3d", _stack([random_3d(5, 1088, 12), random_3d(6, 1088, 40)]), [1088, 1000], {}, False)
    c["geo N=4097 boxes"] = ("one2d", geo(4097), [4097], {}, False)
    c["geo N=4097 matrix"] = ("matrix", geo(4097, 2), [4097], {}, False)
    # cut at the cap: group_size 3, every cluster above 4 members leaves candidates behind (K5 proper: the fast tail gives up); both launch kinds
    c["cap 4 one-launch"] = ("one2d", geo(1000), [1000], dict(group_size=3), False)
    c["cap 4 tail_kernel"] = ("matrix", geo(1088), [1088], dict(group_size=3), False)
    c["cap 4 N=4097"] = ("one2d", geo(4097), [4097], dict(group_size=3), False)
    # runs longer than the halo: 180 members through the fast tail's CSR workgroup; 201 of a cluster of 230 (cut) and 280 (> kFastGroupMax) through K5
    long_sizes = [50, 180, 30, 130, 129, 7]
    c["long fast tail"] = ("matrix", _stack([built(3, 1088, long_sizes)]), [1088], dict(group_size=200), False)
    c["long one-launch"] = ("one2d", _stack([built(3, 1000, long_sizes)]), [1000], dict(group_size=200), False)
    c["long cut K5"] = ("matrix", _stack([built(4, 1088, [50, 230, 30, 280, 5])]), [1088], dict(group_size=200), False)
    c["long > kFastGroupMax"] = ("one2d", _stack([built(4, 1088, [20, 280, 300, 5])]), [1088], dict(group_size=400), False)
    # all singletons / one single run (short enough for the fast tail, and not)
    c["singletons"] = ("one2d", _stack([built(5, 300, []), built(6, 300, [])]), [300, 299], {}, False)
    c["one run 200"] = ("matrix", _stack([built(7, 200, [200])]), [200], dict(group_size=1000), False)
    c["one run 300"] = ("one2d", _stack([built(7, 300, [300])]), [300], dict(group_size=1000), False)
    c["one run 1088"] = ("one2d", _stack([built(7, 1088, [1088])]), [1088], dict(group_size=100000), False)
    # ragged batches: counts 0, 1, N - 1, N with N no multiple of 64 or 256
    for n in (65, 257, 1000):
        imgs = _stack([random_2d(100 * n + b, n, 8) for b in range(4)])
        c[f"ragged {n} boxes"] = ("one2d", imgs, [0, 1, n - 1, n], {}, False)
        c[f"ragged {n} matrix"] = ("matrix", imgs, [n, n - 1, 1, 0], {}, False)
    c["ragged 1090 boxes"] = ("one2d", _stack([random_2d(77 + b, 1090, 24) for b in range(4)]), [1089, 0, 1090, 1], {}, False)
    return c


def _params(lib, kw):
    from groomed_nms_amd._lib import GnmsParams
    P = GnmsParams()
    lib.gnms_default_params(ctypes.byref(P))
    k = dict(DEFAULTS)
    k.update(kw)
    assert k["pruning_method"] == "linear" and k["group_boxes"] and k["mask_group_boxes"] and not k["return_sorted_prob"]
    P.nms_threshold, P.temperature, P.valid_box_prob_threshold, P.group_size = k["nms_threshold"], k["temperature"], k["valid_box_prob_threshold"], k["group_size"]
    return P, k


class Call:
    """the device buffers of one case; forward() and backward() are the C-ABI calls, on `stream`"""

    def __init__(self, lib, case, ws=None, fill=None):
        from groomed_nms_amd._lib import ptr, check
        entry, (src, scores, gp), counts, kw, asym = case
        self.lib, self.entry, self.counts, self.ptr, self.check = lib, entry, counts, ptr, check
        self.P, self.kw = _params(lib, kw)
        dev = torch.device("cuda")
        self.B, self.N = B, N = scores.shape
        self.src, self.scores, self.gp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (src, scores, gp))
        self.ct = torch.tensor(counts, dtype=torch.int32, device=dev)
        self.iou = torch.empty((B, N, N), device=dev)
        if entry == "matrix":
            check(lib.gnms_iou2d(ptr(self.src), ptr(self.src), B, N, N, ptr(self.iou), N, None), "iou2d")
            if asym:
                m = self.iou.cpu().numpy()
                self.iou.copy_(torch.from_numpy(np.stack([asymmetric(m[b], np.random.default_rng(b)) for b in range(B)])))
        self.nbytes = lib.gnms_workspace_bytes(B, N, ctypes.byref(self.P))
        self.ws = ws if ws is not None else torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        assert self.ws.numel() >= self.nbytes
        if fill is not None:
            self.ws.fill_(fill)
        self.prob = torch.full((B, N), float("nan"), device=dev)
        self.valid = torch.empty((B, N), dtype=torch.int64, device=dev)
        self.invalid = torch.empty((B, N), dtype=torch.int64, device=dev)
        self.nv, self.ni = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        self.grad = torch.full((B, N), float("nan"), device=dev)
        self.grad_iou = None

    def forward(self, stream=None):
        lib, ptr, P, B, N = self.lib, self.ptr, self.P, self.B, self.N
        out = (ptr(self.prob), None, ptr(self.valid), ptr(self.invalid), ptr(self.nv), ptr(self.ni), ptr(self.ws), self.ws.numel(), stream)
        if self.entry == "matrix":
            self.check(lib.gnms_forward(ptr(self.scores), ptr(self.iou), B, N, N, ptr(self.ct), ctypes.byref(P), *out), "gnms_forward")
        else:
            fwd = lib.gnms_forward_with_iou2d if self.entry == "one2d" else lib.gnms_forward_with_iou3d
            self.check(fwd(ptr(self.src), ptr(self.scores), B, N, N, ptr(self.ct), ctypes.byref(P), ptr(self.iou), *out), self.entry)

    def backward(self, stream=None, want_grad_iou=False):
        lib, ptr, B, N = self.lib, self.ptr, self.B, self.N
        if want_grad_iou and self.grad_iou is None:
            self.grad_iou = torch.empty((B, N, N), device=self.grad.device)
        gi = ptr(self.grad_iou) if want_grad_iou else None
        self.check(lib.gnms_backward(ptr(self.gp), ptr(self.scores), ptr(self.iou), B, N, N, ptr(self.ct), ctypes.byref(self.P), ptr(self.grad), gi,
                                     ptr(self.ws), self.ws.numel(), stream), "gnms_backward")

    def result(self):
        torch.cuda.synchronize()
        return dict(prob=self.prob.cpu().numpy(), grad=self.grad.cpu().numpy(), valid=self.valid.cpu().numpy(), invalid=self.invalid.cpu().numpy(),
                    nv=self.nv.cpu().numpy(), ni=self.ni.cpu().numpy())


def run_case(lib, case, **kw):
    c = Call(lib, case, **kw)
    c.forward()
    c.backward()
    return c, c.result()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle_image(tag, b):
    """the oracle's result for image b of a case, on the matrix the GPU itself used (computed once, shared by the tests)"""
    from oracle import oracle as O
    case = cases()[tag]
    call = _matrices(tag)
    n = case[2][b]
    _, scores, gp = case[1]
    k = dict(DEFAULTS)
    k.update(case[3])
    ref = O._nms_core(scores[b, :n], np.ascontiguousarray(call[b, :n, :n]), gp[b, :n], True, 0, **k)
    sizes = [len(g) for g in O.get_groups(np.ascontiguousarray(call[b, :n, :n]), k["nms_threshold"], scores[b, :n], k["group_size"])]
    return ref, sizes


@functools.lru_cache(maxsize=4)
def _matrices(tag):
    """[B,N,N] overlaps of a case as the device computed them (the one-call entries write them; bit-identical to the oracle's in 2D)"""
    from groomed_nms_amd import _lib
    c = Call(_lib.load(), cases()[tag])
    c.forward()
    torch.cuda.synchronize()
    return c.iou.cpu().numpy()


def check_against_oracle(tag, res, what=""):
    case = cases()[tag]
    N = case[1][1].shape[1]
    for b, n in enumerate(case[2]):
        t = f"{tag} image {b} n={n} {what}"
        assert not res["grad"][b, n:].any() and not res["prob"][b, n:].any(), f"{t}: padding not zero"
        assert not np.isnan(res["grad"][b]).any(), f"{t}: grad_scores has entries nobody wrote"
        if n == 0:
            continue
        ref, _ = _oracle_image(tag, b)
        bad = np.flatnonzero(res["grad"][b, :n] != ref["grad_scores"])
        assert len(bad) == 0, f"{t}: grad_scores differs from the oracle at {len(bad)} of {n}, first {bad[:5]}: {res['grad'][b, bad[:5]]} vs {ref['grad_scores'][bad[:5]]}"
        assert np.array_equal(res["prob"][b, :n], ref["prob"]), f"{t}: prob"
        assert res["valid"][b, :res["nv"][b]].tolist() == list(ref["valid"]) and res["invalid"][b, :res["ni"][b]].tolist() == list(ref["invalid"]), t
        assert (res["valid"][b, res["nv"][b]:] == -1).all() and (res["invalid"][b, res["ni"][b]:] == -1).all(), t
    assert N >= max(case[2])


@pytest.fixture(scope="module")
def lib():
    from groomed_nms_amd import _lib
    assert torch.cuda.is_available(), "these tests need the GPU"
    assert os.environ.get("GNMS_BWD_PLAN", "1") != "0", "the suite tests the default backward"
    return _lib.load()


_CHILD = """
import sys, numpy as np
sys.path.insert(0, "tests")
from groomed_nms_amd import _lib
import test_backward_plan as T
lib = _lib.load()
np.savez(sys.argv[1], **{tag: T.run_case(lib, case)[1]["grad"] for tag, case in T.cases().items()})
"""


@pytest.fixture(scope="module")
def fused_kernel_grads():
    """grad_scores of every case from bwd_masked_fused_kernel: one fresh child process with GNMS_BWD_PLAN=0"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fused.npz")
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _CHILD, path], cwd=root, env=dict(os.environ, GNMS_BWD_PLAN="0"),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


def test_geometry_is_what_the_cases_claim():
    """the oracle's groups of the built images are the clusters, in the listed order: the runs lie where GEOMETRY's comment puts them"""
    _, sizes = _oracle_image("geo tail_kernel", 0)
    assert sizes[:len(GEOMETRY)] == GEOMETRY and set(sizes[len(GEOMETRY):]) == {1}, sizes[:24]
    starts = np.concatenate([[0], np.cumsum(GEOMETRY)])
    runs = list(zip(starts[:-1], starts[1:]))
    assert any(a < 64 < e for a, e in runs) and any(a < 256 < e for a, e in runs)               # straddle a wave's and a workgroup's boundary
    assert any(e % 256 == 128 for a, e in runs) and any(e % 64 == 0 and e - a > 1 for a, e in runs)   # end exactly on one
    assert any(a % 64 == 0 and e - a == 101 for a, e in runs)                                     # the cap, from a boundary
    _, sizes = _oracle_image("cap 4 tail_kernel", 0)
    assert max(sizes) == 4 and sizes.count(4) >= 10, "group_size + 1 members, the other candidates cut off"
    _, sizes = _oracle_image("long fast tail", 0)
    assert sizes[:5] == [50, 180, 30, 130, 129] and 180 > HALO + 1 and 130 == HALO + 2 and 129 == HALO + 1   # both sides of the halo
    _, sizes = _oracle_image("long cut K5", 0)
    assert sizes[:4] == [50, 201, 30, 201]
    _, sizes = _oracle_image("long > kFastGroupMax", 0)
    assert sizes[:3] == [20, 280, 300]
    assert set(_oracle_image("singletons", 0)[1]) == {1}
    for tag, n in (("one run 200", 200), ("one run 300", 300), ("one run 1088", 1088)):
        assert _oracle_image(tag, 0)[1] == [n], tag
    # clamp saturation on both sides, for heads and for members; dL/dprob with zeros of both signs
    case = cases()["geo tail_kernel"]
    ref, _ = _oracle_image("geo tail_kernel", 0)
    s, gp = case[1][1][0], case[1][2][0]
    pre_sat = ref["grad_scores"] == 0
    assert (s > 1).any() and (s < 0).any() and (gp == 0).sum() > 50 and np.signbit(gp[gp == 0]).any() and (gp < 0).any()
    assert (pre_sat & (gp != 0)).sum() > 100, "saturated clamps"


@pytest.mark.parametrize("tag", list(cases().keys()))
def test_case_against_oracle_and_fused_kernel(lib, fused_kernel_grads, tag):
    _, res = run_case(lib, cases()[tag])
    check_against_oracle(tag, res)
    old = fused_kernel_grads[tag]
    bad = np.flatnonzero(bits(res["grad"]) != bits(old))
    assert len(bad) == 0, f"{tag}: the two backward kernels differ in {len(bad)} words, first {bad[:5]}: {res['grad'].flat[bad[:5]]} vs {old.flat[bad[:5]]}"


@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["ws=00", "ws=ff"])
@pytest.mark.parametrize("tag", ["geo one-launch boxes", "geo tail_kernel", "cap 4 tail_kernel", "ragged 257 matrix", "geo N=4097 boxes"])
def test_stale_workspace_bytes(lib, tag, fill):
    _, res = run_case(lib, cases()[tag], fill=fill)
    check_against_oracle(tag, res, f"workspace filled with {fill:#x}")


def test_workspace_reused_for_a_smaller_shape(lib):
    """one allocation: a large shape's call, then smaller shapes in the same bytes -- every forward writes the whole plan it will read"""
    big, _ = run_case(lib, cases()["geo N=4097 boxes"])
    for tag in ("geo tail_kernel", "long fast tail", "geo one-launch boxes", "ragged 257 boxes", "singletons", "ragged 65 matrix"):
        _, res = run_case(lib, cases()[tag], ws=big.ws)
        check_against_oracle(tag, res, "in a larger shape's workspace")


@pytest.mark.parametrize("tag", ["geo tail_kernel", "long cut K5", "ragged 257 boxes"])
def test_two_backwards_from_one_forward(lib, tag):
    """with and without dL/diou (gx is stored only for the matrix gradient's kernel): the same grad_scores, and the matrix gradient the oracle's"""
    c, first = run_case(lib, cases()[tag])
    c.grad.fill_(float("nan"))
    c.backward(want_grad_iou=True)
    second = c.result()
    assert np.array_equal(bits(first["grad"]), bits(second["grad"]))
    check_against_oracle(tag, second, "second backward")
    gi = c.grad_iou.cpu().numpy()
    for b, n in enumerate(cases()[tag][2]):
        assert not gi[b, n:].any() and not gi[b, :, n:].any()
        if n > 1:
            ref, _ = _oracle_image(tag, b)
            assert np.array_equal(gi[b, :n, :n], ref["grad_iou"]), f"{tag} image {b}: grad_iou"
    c.grad.fill_(float("nan"))
    c.backward()
    assert np.array_equal(bits(first["grad"]), bits(c.result()["grad"]))


@pytest.mark.parametrize("tag", ["geo one-launch boxes", "geo writer launch 2D", "ragged 1000 matrix"])
def test_step_in_a_graph_replayed(lib, tag):
    c, eager = run_case(lib, cases()[tag])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        c.forward(sp)
        c.backward(sp)
    for rep in range(3):
        c.grad.fill_(float("nan"))
        c.prob.fill_(float("nan"))
        graph.replay()
        res = c.result()
        assert np.array_equal(bits(res["grad"]), bits(eager["grad"])), f"{tag}: replay {rep}"
        check_against_oracle(tag, res, f"replay {rep}")
