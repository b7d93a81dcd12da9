"""The optimiser side of the reference's loop on the GPU (lib/core.py:99-170; csrc/optim.hip): what stands between
RPN_3D_loss.forward_packed + backward and a training step that is captured as a whole.

  lr_schedule     conf -> float64 [max_iter]: the value the reference's adjust_lr sets at every iteration, with the reference's
                  expressions in the reference's order on the host (poly with lr_power, step with lr_steps, warmup): bit for bit.
  adjust_lr       lib/core.py:116-170 with its signature, from that schedule (cached per configuration); get_lr beside it.
  FusedSGD        a torch.optim.Optimizer whose step is ONE launch per parameter group (gnms_sgd_step): clip_grad_value_, weight
                  decay, momentum, the update and zero_grad, float32, every operation rounded on its own.  step(loss=...) applies
                  `if loss > 0` (lib/core.py:102) on the device; with capturable=True the learning rate comes from a device copy of
                  the schedule, indexed by an iteration counter the launch advances itself: nothing is read on the host.  The state
                  is {'momentum_buffer': tensor} per parameter, so state_dict() / load_state_dict() interchange with torch.optim.SGD.
  loss_backprop   lib/core.py:99-113 with its signature: loss.backward(), then optimizer.step(loss=loss).
  plan            the pure host function that cuts the tensors of a group into the kernel's tasks.

Deliberate differences from the reference:
  * The gate.  The reference reads the loss on the host and, unless loss > 0, skips backward, the clip and the step.  Here backward
    has already run; the kernel then discards its result: p and buf stay bit for bit as they were and g is zeroed.  With the
    reference's zero_grad after every step the state afterwards is the same; BatchNorm's running statistics and anything else the
    forward pass changed are as in the reference, which ran that forward pass too.
  * buf = mo * buf + d from a buffer of zeros, where torch clones d at the first step: a clipped gradient of -0.0 (and wd * p = +-0)
    leaves +0.0 in buf where torch leaves -0.0.  The parameter is the same either way.
  * A parameter that requires a gradient and has none is given one of zeros, once, so that the addresses the launch reads stay the
    same from step to step; it then takes part in every step (weight decay and momentum included), where torch.optim.SGD passes over
    a parameter whose .grad is None.  After the reference's first zero_grad() its gradients are zeros, not None, as well.
  * momentum = 0 keeps a buffer as well (it holds d); torch keeps none.
  * batch_skip > 1 is not implemented: the device gate cannot take one micro-step's gradient out of the sum again.

Supported: float32 contiguous dense parameters on one device; dampening = 0, no nesterov, no maximize.  There is no CPU
implementation: without a GPU step() raises _lib.GnmsError.
"""
import collections.abc

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

__all__ = ["lr_schedule", "adjust_lr", "get_lr", "FusedSGD", "loss_backprop", "plan", "CHUNK"]

CHUNK = 8192                                         # elements of one task: 32 KiB per stream, 8 passes of a 256-thread workgroup
_ROW = 4                                             # GNMS_SGD_ROW
VECTOR, SCALAR = 1, 0                                # a task's kind

# measurement variants (tools/optim_time.py): workgroups of the launch (0: the library's choice), and which of the 16-byte accesses are
# non-temporal (bit 0: the loads, bit 1: the stores)
GRID = 0
NONTEMPORAL = 0


# ------------------------------------------------------------------------------------------------ the schedule (host)
def _has(conf, key):
    return key in conf if isinstance(conf, collections.abc.Mapping) else hasattr(conf, key)


def _get(conf, key):
    return conf[key] if isinstance(conf, collections.abc.Mapping) else getattr(conf, key)


def _check_solver(conf):
    if str(_get(conf, "solver_type")).lower() != "sgd":
        raise NotImplementedError("solver_type %r: only 'sgd' is implemented (lib/core.py:80-93 has adam and adamax)" % (_get(conf, "solver_type"),))


def _lr_at(conf, iter):
    """lib/core.py:131-162 as it stands: the operand types are the reference's too (np.int64 step counts, Python floats)"""
    lr = _get(conf, "lr")
    lr_steps = _get(conf, "lr_steps")
    max_iter = _get(conf, "max_iter")
    lr_policy = _get(conf, "lr_policy")
    lr_target = _get(conf, "lr_target")

    if lr_steps:
        steps = np.array(lr_steps) * max_iter
        total_steps = steps.shape[0]
        step_count = np.sum((steps - iter) <= 0)
    else:
        total_steps = max_iter
        step_count = iter

    warmup = None if not _has(conf, "warmup") else _get(conf, "warmup")
    if warmup is not None and step_count <= warmup:
        scale = (step_count + 1) / float(warmup)
        lr *= scale
    elif lr_policy.lower() == "step":
        scale = (lr_target / lr) ** (1 / total_steps)
        lr *= scale ** step_count
    elif lr_policy.lower() == "poly":
        power = 0.9 if not _has(conf, "lr_power") else _get(conf, "lr_power")
        scale = total_steps / (1 - (lr_target / lr) ** (1 / power))
        lr *= (1 - step_count / scale) ** power
    else:
        raise ValueError("{} lr_policy not understood".format(lr_policy))
    return lr


def _schedule_key(conf):
    steps = _get(conf, "lr_steps")
    return (float(_get(conf, "lr")), tuple(steps) if steps else None, int(_get(conf, "max_iter")), str(_get(conf, "lr_policy")),
            float(_get(conf, "lr_target")), _get(conf, "warmup") if _has(conf, "warmup") else None,
            _get(conf, "lr_power") if _has(conf, "lr_power") else None)


_SCHEDULES = {}


def lr_schedule(conf):
    """float64 [max_iter]: entry i is what the reference's adjust_lr(conf, optimizer, i) writes into param_group['lr']"""
    _check_solver(conf)
    key = _schedule_key(conf)
    table = _SCHEDULES.get(key)
    if table is None:
        table = np.array([_lr_at(conf, i) for i in range(int(_get(conf, "max_iter")))], dtype=np.float64)
        table.setflags(write=False)
        if len(_SCHEDULES) >= 8:
            _SCHEDULES.clear()
        _SCHEDULES[key] = table
    return table


def adjust_lr(conf, optimizer, iter):
    """lib/core.py:116-170: sets every param_group['lr'] to the schedule's value at `iter` (past max_iter: the same expressions)"""
    if _has(conf, "batch_skip") and ((iter + 1) % _get(conf, "batch_skip")) > 0:
        return
    table = lr_schedule(conf)
    lr = float(table[iter]) if 0 <= iter < table.shape[0] else float(_lr_at(conf, iter))
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr


def get_lr(optimizer):
    for param_group in optimizer.param_groups:
        return param_group["lr"]


# ------------------------------------------------------------------------------------------------ the planner (host)
def plan(numels, byte_offsets, chunk=CHUNK):
    """numels[i]: elements of tensor i; byte_offsets[i]: the byte address (or offset from a 16-byte boundary) of its p, g and buf, one
    int where the three are the same or a triple.  Returns (tensors int64 [T, 4] = p, g, buf, numel; tasks int64 [n, 4] = tensor,
    start, count, kind).  Every element lies in exactly one task, no task crosses a tensor or exceeds `chunk` elements, and a VECTOR task
    starts where all three arrays are on 16 bytes; where they share a misalignment the elements before the first boundary are a
    SCALAR task of their own, and where they do not the whole tensor is cut into SCALAR tasks."""
    chunk = int(chunk)
    if chunk < 4 or chunk % 4:
        raise ValueError("chunk=%r: a positive multiple of 4 elements" % (chunk,))
    if len(numels) != len(byte_offsets):
        raise ValueError("%d element counts for %d offsets" % (len(numels), len(byte_offsets)))
    tensors = np.zeros((len(numels), _ROW), np.int64)
    tasks = []
    for i, (n, off) in enumerate(zip(numels, byte_offsets)):
        n = int(n)
        trio = tuple(int(o) for o in off) if isinstance(off, (tuple, list, np.ndarray)) else (int(off),) * 3
        if n < 0 or len(trio) != 3:
            raise ValueError("tensor %d: numel=%r byte_offsets=%r" % (i, n, off))
        if any(o % 4 for o in trio):
            raise ValueError("tensor %d: float32 data at byte offsets %r" % (i, trio))
        tensors[i] = trio + (n,)
        mis = {o % 16 for o in trio}
        start = 0
        if len(mis) == 1:
            head = min(n, (16 - mis.pop()) % 16 // 4)
            if head:
                tasks.append((i, 0, head, SCALAR))
                start = head
            kind = VECTOR
        else:
            kind = SCALAR
        while start < n:
            count = min(chunk, n - start)
            tasks.append((i, start, count, kind))
            start += count
    return tensors, np.array(tasks, np.int64).reshape(-1, _ROW)


# ------------------------------------------------------------------------------------------------ the optimiser
class _Group:
    """what one parameter group's launch reads: the tensors in table order, the device tables, and the identity they were built for"""
    __slots__ = ("params", "grads", "bufs", "versions", "key", "tensors", "tasks", "n_tensors", "n_tasks")


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0, weight_decay=0, *, dampening=0, nesterov=False, maximize=False, clip_value=1.0,
                 lr_table=None, capturable=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if clip_value is not None and not clip_value >= 0:
            raise ValueError("Invalid clip_value: %r (>= 0, or None for no clip)" % (clip_value,))
        if capturable and lr_table is None:
            raise ValueError("capturable=True takes the learning rate from lr_table (optim.lr_schedule(conf))")
        # every key torch.optim.SGD reads from a group, so that a state_dict() of this loads into it
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=None, differentiable=False, fused=None, clip_value=clip_value)
        super().__init__(params, defaults)
        self.capturable = bool(capturable)
        self.lr_table = None if lr_table is None else np.array(lr_table, dtype=np.float64).reshape(-1)
        if self.lr_table is not None and self.lr_table.shape[0] < 1:
            raise ValueError("lr_table is empty")
        self.launches = 0                              # device launches this optimiser has issued (step and zero_grad)
        self._plans = None                             # one _Group per param_group, built by prepare()
        self._device = None
        self._state = None                             # int64 [2] on the device: iteration, ticket
        self._lr_dev = None
        self._iteration = 0                            # until the device counter exists
        self._zeroed = False                           # the last step left every gradient zero
        self._validate()

    # ---- arguments
    def _validate(self):
        for group in self.param_groups:
            if group.get("dampening", 0) != 0:
                raise NotImplementedError("dampening=%r is not implemented" % (group["dampening"],))
            if group.get("nesterov", False):
                raise NotImplementedError("nesterov momentum is not implemented")
            if group.get("maximize", False):
                raise NotImplementedError("maximize is not implemented")
            if group.get("differentiable", False):
                raise NotImplementedError("differentiable is not implemented")
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise NotImplementedError("a %s parameter: only float32 parameters are implemented (no mixed precision)" % (p.dtype,))
                if p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError("a non-contiguous parameter of shape %r, strides %r" % (tuple(p.shape), tuple(p.stride())))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plans = None
        if hasattr(self, "launches"):
            self._validate()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = None
        self._zeroed = False
        self._validate()

    # ---- the iteration counter
    def set_iteration(self, n):
        self._iteration = int(n)
        if self._state is not None:
            self._state.copy_(torch.tensor([int(n), 0], dtype=torch.int64))

    def iteration(self):
        """the counter as the device holds it (a host read: for logging and checkpoints, not for the step)"""
        return self._iteration if self._state is None else int(self._state[0].item())

    # ---- tables
    def _live(self, group):
        return [p for p in group["params"] if p.requires_grad]

    def prepare(self):
        """Materialises missing gradients and momentum buffers as zeros and builds the device tables.  step() does it when the set of
        tensors or an address has changed; call it (or take one step) before capturing a graph."""
        if not torch.cuda.is_available():
            raise _lib.GnmsError("FusedSGD needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedSGD: a gradient, parameter or momentum buffer has moved (or prepare() never ran) while a graph is being "
                               "captured; call prepare() before the capture and keep the tensors")
        device = None
        for group in self.param_groups:
            for p in group["params"]:
                if not p.is_cuda:
                    raise _lib.GnmsError("FusedSGD: a parameter on %s; there is no CPU implementation" % (p.device,))
                if device is not None and p.device != device:
                    raise ValueError("FusedSGD: parameters on %s and %s" % (device, p.device))
                device = p.device
        self._validate()
        plans = []
        for group in self.param_groups:
            g = _Group()
            g.params = self._live(group)
            g.grads, g.bufs = [], []
            for p in g.params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
                grad = p.grad
                if grad.layout != torch.strided:
                    raise ValueError("a sparse gradient (parameter of shape %r)" % (tuple(p.shape),))
                if grad.dtype != torch.float32 or grad.device != p.device or grad.shape != p.shape:
                    raise ValueError("a gradient of %s %r on %s for a float32 parameter of shape %r" % (grad.dtype, tuple(grad.shape), grad.device, tuple(p.shape)))
                if not grad.is_contiguous():
                    raise ValueError("a non-contiguous gradient of shape %r, strides %r" % (tuple(grad.shape), tuple(grad.stride())))
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None:
                    buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if buf.dtype != torch.float32 or buf.device != p.device or buf.shape != p.shape or not buf.is_contiguous():
                    raise ValueError("a momentum buffer of %s %r for a float32 parameter of shape %r" % (buf.dtype, tuple(buf.shape), tuple(p.shape)))
                g.grads.append(grad)
                g.bufs.append(buf)
            numels = [p.numel() for p in g.params]
            if any(n >= 1 << 40 for n in numels):
                raise ValueError("a parameter of more than 2^40 elements")
            addresses = [(p.data_ptr(), gr.data_ptr(), b.data_ptr()) for p, gr, b in zip(g.params, g.grads, g.bufs)]
            tensors, tasks = plan(numels, addresses, CHUNK)
            g.n_tensors, g.n_tasks = int(tensors.shape[0]), int(tasks.shape[0])
            both = torch.from_numpy(np.concatenate([tensors.reshape(-1), tasks.reshape(-1)])).to(device) if device is not None else None
            g.tensors = both[:tensors.size] if g.n_tensors else None
            g.tasks = both[tensors.size:] if g.n_tasks else None
            g.key = [a for trio in addresses for a in trio[:2]]
            g.versions = None
            plans.append(g)
        if device is not None and (self._state is None or self._state.device != device):
            self._state = torch.tensor([self._iteration, 0], dtype=torch.int64).to(device)
            self._lr_dev = None if self.lr_table is None else torch.from_numpy(self.lr_table).to(device)
        self._device = device
        self._plans = plans

    def _current(self):
        """the cheap per-step check: the same parameters with a gradient, at the same addresses, with the same buffers"""
        plans = self._plans
        if plans is None or len(plans) != len(self.param_groups):
            return False
        try:
            for group, g in zip(self.param_groups, plans):
                key = []
                for p in group["params"]:
                    if p.requires_grad:
                        key.append(p.data_ptr())
                        key.append(p.grad.data_ptr())
                if key != g.key:
                    return False
                for p, buf in zip(g.params, g.bufs):
                    if self.state[p].get("momentum_buffer") is not buf:
                        return False
        except (AttributeError, RuntimeError):         # a gradient that is None, or sparse
            return False
        return True

    # ---- the step
    @torch.no_grad()
    def step(self, loss=None):
        """One launch per parameter group.  loss: None (no gate), or a zero-dimensional tensor on the parameters' device; it is read
        by the kernel, never on the host."""
        if callable(loss):
            raise NotImplementedError("closure: FusedSGD.step takes the loss tensor, not a closure")
        if not self._current():
            self.prepare()
        if self._device is None:
            return None
        gate = None
        if loss is not None:
            if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
                raise ValueError("loss must be a tensor of one element")
            if loss.device != self._device:
                raise ValueError("loss on %s, parameters on %s" % (loss.device, self._device))
            gate = loss.detach()
            if gate.dtype != torch.float32:
                gate = gate.to(torch.float32)
        lib = _lib.load()
        table, table_len = (ptr(self._lr_dev), int(self._lr_dev.shape[0])) if self.capturable else (None, 0)
        last = len(self._plans) - 1
        with _lib.on_device(self._device):
            stream = stream_ptr(self._device)
            for i, (group, g) in enumerate(zip(self.param_groups, self._plans)):
                if g.n_tasks == 0 and i != last:
                    continue
                clip = group.get("clip_value", self.defaults["clip_value"])
                check(lib.gnms_sgd_step(ptr(g.tensors), g.n_tensors, ptr(g.tasks), g.n_tasks, group["lr"], group["momentum"],
                                        group["weight_decay"], 0.0 if clip is None else clip, 0 if clip is None else 1, ptr(gate),
                                        table, table_len, ptr(self._state), 1 if i == last else 0, GRID, int(NONTEMPORAL) & 3, stream),
                      "gnms_sgd_step")
                self.launches += 1
        for g in self._plans:
            g.versions = [grad._version for grad in g.grads]
        self._zeroed = True
        return None

    def zero_grad(self, set_to_none=False):
        """The reference's optimizer.zero_grad() after step(): the step has zeroed the gradients already, and where nothing has written
        to them since (same tensors, same version counters) this launches nothing.  The tensors are kept unless set_to_none."""
        if set_to_none:
            self._zeroed = False
            return super().zero_grad(set_to_none=True)
        if self._zeroed and self._plans is not None and self._current() and all(
                g.versions is not None and all(grad._version == v for grad, v in zip(g.grads, g.versions)) for g in self._plans):
            return None
        self._zeroed = False
        grads = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    p.grad.requires_grad_(False)
                    grads.append(p.grad)
        if grads:
            torch._foreach_zero_(grads)
            self.launches += 1
        return None


def loss_backprop(loss, net, optimizer, conf=None, iteration=None):
    """lib/core.py:99-113 without its host read: backward always runs, and the step applies `loss > 0` on the device."""
    if conf is not None and _has(conf, "batch_skip") and _get(conf, "batch_skip") > 1:
        raise NotImplementedError("batch_skip=%r: gradient accumulation over skipped steps is not implemented" % (_get(conf, "batch_skip"),))
    loss.backward()
    if conf is None or iteration is None:
        torch.nn.utils.clip_grad_value_(net.parameters(), 1)
        return
    optimizer.step(loss=loss)
