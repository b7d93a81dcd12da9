"""Generate tests/golden/optim.npz by IMPORTING the reference's lib/core.py and running its own adjust_lr over whole schedules and its
own loss_backprop (clip_grad_value_ + torch.optim.SGD.step + zero_grad, behind `if loss > 0`) on the CPU over a few iterations of a
tiny model built here.  Runs only where the reference checkout is (the first argument, read-only); it writes data only: the
configurations, the learning rates, and per iteration the raw gradients, the loss, and the parameters and momentum buffers afterwards.

lib/core.py imports easydict, shapely, matplotlib and cv2 at module top; none of them is used by these two functions, so those that
are missing are stubbed.  usage: python tests/golden/make_optim_golden.py REFERENCE_CHECKOUT"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "optim.npz")

LR = 0.004                                             # scripts/config/*.py
SCHEDULES = {
    "poly": dict(solver_type="sgd", lr=LR, lr_policy="poly", lr_steps=None, lr_target=LR * 0.00001, max_iter=300),
    "poly_power": dict(solver_type="sgd", lr=LR, lr_policy="poly", lr_power=0.7, lr_steps=None, lr_target=LR * 0.00001, max_iter=250),
    "step": dict(solver_type="sgd", lr=LR, lr_policy="step", lr_steps=[0.3, 0.6, 0.85], lr_target=LR * 0.001, max_iter=200),
    "warmup": dict(solver_type="sgd", lr=LR, lr_policy="poly", lr_steps=None, lr_target=LR * 0.00001, max_iter=300, warmup=25),
}
# the tiny model: a scalar, sizes around one 16-byte vector, a matrix, and a vector that is no multiple of 4
SHAPES = ((1,), (3,), (4,), (5,), (33, 5), (1031,))
TRAIN = dict(solver_type="sgd", lr=LR, momentum=0.9, weight_decay=0.0005, lr_policy="poly", lr_steps=None, lr_target=LR * 0.00001, max_iter=50)
LOSSES = (2.5, 0.75, 0.0, 1.25, -1.0, 0.5)             # iterations 2 and 4 are gated (loss <= 0)
GRAD_SCALES = (0.3, 3.0, 3.0, 0.3, 3.0, 3.0)           # 3.0: a third of the gradients lie beyond +-1


class _Stub(types.ModuleType):
    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return object


class Obj(dict):
    """what easydict gives the reference: keys as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def load_reference():
    names = []
    for name in ("easydict", "shapely", "shapely.geometry", "matplotlib", "matplotlib.pyplot", "cv2", "visdom", "torchvision",
                 "torchvision.transforms", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:                                                                 # noqa: BLE001
            names.append(name)
    for name in names:
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    import lib.core as core           # noqa: E402
    return core


class Tiny(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


def main():
    if REF is None:
        sys.exit(__doc__)
    core = load_reference()
    z = {"torch_version": np.array(torch.__version__), "numpy_version": np.array(np.__version__)}

    # ---- the schedules: the reference's adjust_lr at every iteration
    z["schedules"] = np.array(sorted(SCHEDULES))
    for name, settings in SCHEDULES.items():
        conf = Obj(settings)
        probe = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=conf.lr)
        lrs = []
        for it in range(conf.max_iter):
            core.adjust_lr(conf, probe, it)
            lrs.append(core.get_lr(probe))
        z["sched/%s/conf" % name] = np.array(json.dumps(settings))
        z["sched/%s/lr" % name] = np.array(lrs, dtype=np.float64)

    # ---- the step: the reference's loss_backprop on the CPU
    gen = torch.Generator().manual_seed(20)
    init = [torch.randn(s, generator=gen) * 0.1 for s in SHAPES]
    net = Tiny(init)
    params = list(net.parameters())
    conf = Obj(TRAIN)
    optimizer = torch.optim.SGD(net.parameters(), lr=conf.lr, momentum=conf.momentum, weight_decay=conf.weight_decay)   # lib/core.py:77
    z["train/conf"] = np.array(json.dumps(TRAIN))
    z["train/n_iter"] = np.array(len(LOSSES))
    z["train/n_tensors"] = np.array(len(SHAPES))
    for k, t in enumerate(init):
        z["train/init/%d" % k] = t.numpy().copy()
    for it, (value, scale) in enumerate(zip(LOSSES, GRAD_SCALES)):
        core.adjust_lr(conf, optimizer, it)
        z["train/%d/lr" % it] = np.array(core.get_lr(optimizer), dtype=np.float64)
        coeff = [torch.randn(s, generator=gen) * scale for s in SHAPES]
        dot = sum((p * c).sum() for p, c in zip(params, coeff))
        loss = dot - dot.detach() + value                                                 # d loss / d p = coeff; the value is exact
        assert float(loss) == value
        raw = torch.autograd.grad(loss, params, retain_graph=True)
        core.loss_backprop(loss, net, optimizer, conf=conf, iteration=it)
        z["train/%d/loss" % it] = np.array(value, dtype=np.float32)
        for k, p in enumerate(params):
            assert torch.equal(raw[k], coeff[k])
            z["train/%d/grad/%d" % (it, k)] = raw[k].numpy().copy()
            z["train/%d/param/%d" % (it, k)] = p.detach().numpy().copy()
            buf = optimizer.state[p].get("momentum_buffer") if p in optimizer.state else None
            z["train/%d/buf/%d" % (it, k)] = np.zeros(p.shape, np.float32) if buf is None else buf.numpy().copy()
    beyond = sum(int((np.abs(z["train/1/grad/%d" % k]) > 1).sum()) for k in range(len(SHAPES)))
    assert beyond > 100 and any(v <= 0 for v in LOSSES)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
