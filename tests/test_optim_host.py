"""Host side of groomed_nms_amd.optim (no GPU): the schedule against the reference's own adjust_lr (tests/golden/optim.npz, made by
tests/golden/make_optim_golden.py), the planner, the argument errors and the C symbol."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import Golden, ROOT

SCHEDULES = ("poly", "poly_power", "step", "warmup")


class AttrDict(dict):
    """what easydict gives the reference: keys as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


_GOLDEN = []


def golden():
    if not _GOLDEN:
        _GOLDEN.append(Golden("optim.npz"))
    return _GOLDEN[0]


def conf_of(z, key):
    return AttrDict(json.loads(str(z[key])))


@pytest.fixture(scope="module")
def O():
    from groomed_nms_amd import optim
    return optim


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_golden_is_what_the_issue_asks_for():
    z = golden()
    assert sorted(str(s) for s in z["schedules"]) == sorted(SCHEDULES)
    poly = conf_of(z, "sched/poly/conf")
    assert poly.lr == 0.004 and poly.lr_target == poly.lr * 0.00001 and 100 <= poly.max_iter <= 1000
    assert conf_of(z, "sched/step/conf").lr_steps and conf_of(z, "sched/warmup/conf").warmup > 0
    n, T = int(z["train/n_iter"]), int(z["train/n_tensors"])
    losses = [float(z["train/%d/loss" % i]) for i in range(n)]
    assert n >= 5 and any(v <= 0 for v in losses) and losses[0] > 0
    assert max(float(np.abs(z["train/%d/grad/%d" % (i, k)]).max()) for i in range(n) for k in range(T)) > 1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "optim.npz")) < 1 << 19


@pytest.mark.parametrize("name", SCHEDULES)
def test_lr_schedule_is_the_reference_bit_for_bit(O, name):
    z = golden()
    conf = conf_of(z, "sched/%s/conf" % name)
    want = z["sched/%s/lr" % name]
    got = O.lr_schedule(conf)
    assert got.dtype == np.float64 and got.shape == (conf.max_iter,) == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert O.lr_schedule(dict(conf)) is got                                               # cached per configuration, a plain dict too
    if name == "warmup":                                                                  # the boundary: step_count <= warmup, then poly
        w = conf.warmup
        assert got[w] == conf.lr * ((w + 1) / float(w)) and got[w + 1] < conf.lr and got[0] == conf.lr * (1 / float(w))
    if name == "step":
        assert len(np.unique(got)) == len(conf.lr_steps) + 1


@pytest.mark.parametrize("name", SCHEDULES)
def test_adjust_lr_sets_every_group(O, name):
    z = golden()
    conf = conf_of(z, "sched/%s/conf" % name)
    want = z["sched/%s/lr" % name]
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([{"params": [a]}, {"params": [b], "lr": 1.0}], lr=conf.lr, momentum=0.9)
    for it in (0, 1, conf.max_iter // 2, conf.max_iter - 1) + ((conf.warmup, conf.warmup + 1) if name == "warmup" else ()):
        O.adjust_lr(conf, opt, it)
        for group in opt.param_groups:
            assert isinstance(group["lr"], float) and np.float64(group["lr"]).view(np.uint64) == want[it].view(np.uint64)
        assert O.get_lr(opt) == want[it]
    skip = AttrDict(conf, batch_skip=2)                                                   # lib/core.py:127: nothing on the skipped iterations
    opt.param_groups[0]["lr"] = -1.0
    O.adjust_lr(skip, opt, 4)
    assert opt.param_groups[0]["lr"] == -1.0
    O.adjust_lr(skip, opt, 5)
    assert opt.param_groups[0]["lr"] == want[5]


def test_schedule_errors(O):
    conf = conf_of(golden(), "sched/poly/conf")
    with pytest.raises(NotImplementedError, match="solver_type"):
        O.lr_schedule(AttrDict(conf, solver_type="adam"))
    with pytest.raises(NotImplementedError, match="solver_type"):
        O.adjust_lr(AttrDict(conf, solver_type="adam"), None, 0)
    with pytest.raises(ValueError, match="lr_policy not understood"):                      # the reference's own message
        O.lr_schedule(AttrDict(conf, lr_policy="cosine"))


CHUNK = 64


def plan_inputs():
    numels = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
    cases = {
        "aligned": [0] * len(numels),
        "shared_misalignment": [4, 8, 12, 4, 8, 12, 4, 8],
        "mixed": [(0, 4, 0), 0, (8, 8, 12), 12, (4, 0, 0), 0, 4, (12, 0, 4)],
        "addresses": [0x7f0000000000 + 512 * i + (4 if i % 3 == 0 else 0) for i in range(len(numels))],
    }
    return numels, cases


@pytest.mark.parametrize("case", ["aligned", "shared_misalignment", "mixed", "addresses"])
def test_plan_covers_every_element_once(O, case):
    numels, cases = plan_inputs()
    offsets = cases[case]
    tensors, tasks = O.plan(numels, offsets, CHUNK)
    check_plan(O, numels, offsets, tensors, tasks, CHUNK)
    if case == "aligned":                                                                 # nothing but whole chunks and one tail per tensor
        assert tasks[:, 3].tolist() == [O.VECTOR] * len(tasks) and len(tasks) == sum(-(-n // CHUNK) for n in numels)


def test_plan_of_400_single_elements(O):
    numels = [1] * 400
    for offsets in ([0] * 400, [4 * (i % 4) for i in range(400)], [(0, 4, 8)] * 400):
        tensors, tasks = O.plan(numels, offsets, CHUNK)
        check_plan(O, numels, offsets, tensors, tasks, CHUNK)
        assert len(tasks) == 400 and tasks[:, 0].tolist() == list(range(400))


def check_plan(O, numels, offsets, tensors, tasks, chunk):
    assert tensors.dtype == np.int64 and tasks.dtype == np.int64 and tensors.shape == (len(numels), 4) and tasks.shape[1] == 4
    trios = [tuple(o) if isinstance(o, tuple) else (o,) * 3 for o in offsets]
    assert tensors[:, 3].tolist() == list(numels) and [tuple(r) for r in tensors[:, :3].tolist()] == trios
    seen = [np.zeros(n, np.int64) for n in numels]
    for ti, start, count, kind in tasks.tolist():
        assert 0 <= ti < len(numels) and count >= 1 and count <= chunk
        assert 0 <= start and start + count <= numels[ti]                                  # no task crosses its tensor
        seen[ti][start:start + count] += 1
        assert kind in (O.VECTOR, O.SCALAR)
        if kind == O.VECTOR:
            assert all((o + 4 * start) % 16 == 0 for o in trios[ti])                       # vector tasks start on 16 bytes
        if len({o % 16 for o in trios[ti]}) > 1:
            assert kind == O.SCALAR
    assert all((s == 1).all() for s in seen)                                               # every element in exactly one task
    for ti, trio in enumerate(trios):                                                      # and the scalar share of an alignable tensor is its head
        if len({o % 16 for o in trio}) == 1:
            scalar = sum(c for t, s, c, k in tasks.tolist() if t == ti and k == O.SCALAR)
            assert scalar == min(numels[ti], (16 - trio[0] % 16) % 16 // 4)


def test_plan_errors(O):
    with pytest.raises(ValueError):
        O.plan([4], [0], 6)
    with pytest.raises(ValueError):
        O.plan([4, 4], [0], 64)
    with pytest.raises(ValueError):
        O.plan([4], [2], 64)


def test_argument_errors(O):
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(NotImplementedError, match="nesterov"):
        O.FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(NotImplementedError, match="dampening"):
        O.FusedSGD([p], lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(NotImplementedError, match="maximize"):
        O.FusedSGD([p], lr=0.1, maximize=True)
    with pytest.raises(NotImplementedError, match="float16"):
        O.FusedSGD([torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))], lr=0.1)
    with pytest.raises(ValueError, match="non-contiguous"):
        O.FusedSGD([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1)
    with pytest.raises(ValueError):
        O.FusedSGD([p], lr=-0.1)
    with pytest.raises(ValueError, match="lr_table"):
        O.FusedSGD([p], lr=0.1, capturable=True)
    net = torch.nn.Linear(2, 1)
    opt = O.FusedSGD(net.parameters(), lr=0.1, momentum=0.9)
    loss = net(torch.ones(1, 2)).sum()
    with pytest.raises(NotImplementedError, match="batch_skip"):
        O.loss_backprop(loss, net, opt, conf=AttrDict(batch_skip=2), iteration=0)
    assert all(q.grad is None for q in net.parameters())                                   # raised before backward
    with pytest.raises(NotImplementedError, match="closure"):
        opt.step(lambda: None)


def test_state_and_groups_are_torch_sgd_s(O):
    """the keys torch.optim.SGD reads from a group are all there, so a state_dict() of one loads into the other (host side: no step)"""
    a, b = torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3))
    fused = O.FusedSGD([a, b], lr=0.004, momentum=0.9, weight_decay=0.0005)
    sgd = torch.optim.SGD([a, b], lr=0.1, momentum=0.5)
    assert set(sgd.param_groups[0]) <= set(fused.param_groups[0])
    sgd.load_state_dict(fused.state_dict())
    assert sgd.param_groups[0]["lr"] == 0.004 and sgd.param_groups[0]["momentum"] == 0.9
    a.grad, b.grad = torch.ones(5), torch.ones(3)
    sgd.step()                                                                            # torch's own step on the loaded groups
    fused.load_state_dict(sgd.state_dict())
    assert fused.param_groups[0]["weight_decay"] == 0.0005
    assert set(fused.state[a]) == {"momentum_buffer"} and torch.equal(fused.state[a]["momentum_buffer"], sgd.state[a]["momentum_buffer"])


def test_there_is_no_cpu_step(O):
    from groomed_nms_amd import _lib
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = O.FusedSGD([p], lr=0.1)
    with pytest.raises(_lib.GnmsError):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8))


def test_symbol_is_exported_with_the_declared_types(O):
    from groomed_nms_amd import _lib
    lib = _lib.load()
    fn = lib.gnms_sgd_step
    assert "gnms_sgd_step" in _lib.EXPORTED_SYMBOLS and fn.restype is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "groomed_nms_hip.h")).read()
    m = re.search(r"int gnms_sgd_step\(([^;]*)\);", header)
    assert m, "gnms_sgd_step is not declared in include/groomed_nms_hip.h"
    declared = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
    ctype = {"double": ctypes.c_double, "int": ctypes.c_int}
    want = [ctypes.c_void_p if d.endswith("*") else ctype[d] for d in declared]
    assert len(want) == 17 and list(fn.argtypes) == want
    assert declared[0] == "const int64_t*" and declared[9] == "const float*" and declared[10] == "const double*" and declared[12] == "int64_t*"
    import groomed_nms_amd
    assert groomed_nms_amd.optim is O and groomed_nms_amd.FusedSGD is O.FusedSGD and "groomed_nms_amd.optim" in groomed_nms_amd.__doc__
