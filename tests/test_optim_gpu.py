"""groomed_nms_amd.optim.FusedSGD on the GPU (csrc/optim.hip, gnms_sgd_step): bit identity with a NumPy float32 restatement of the five
lines of the step, the reference's own loss_backprop (tests/golden/optim.npz) within twice its own float32 error, the device gate, the
captured step with the schedule on the device, checkpoint interchange with torch.optim.SGD and the reference-shaped call sequence.

NaN: a NaN gradient makes buf and p NaN on both sides; which NaN (sign, payload) is the hardware's choice, so two NaNs compare equal
here and every other value is compared by its bits."""
import copy

import numpy as np
import pytest
import torch

import test_optim_host as H

pytestmark = pytest.mark.gpu

MO, WD = 0.9, 0.0005
f32 = np.float32


@pytest.fixture(scope="module")
def O():
    from groomed_nms_amd import _lib, optim
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the GPU"
    return optim


def lr_at(i):
    return 0.004 * (1 - i / 50.) ** 0.9


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def restate(P, G, B, lr, mo=MO, wd=WD, c=1.0, loss=None):
    """the five lines of the step in float32, one rounding per operation; returns the new (P, B).  G = 0 afterwards either way."""
    if loss is not None and not (f32(loss) > 0):
        return P, B
    with np.errstate(invalid="ignore"):
        g = G if c is None else np.where(G < f32(-c), f32(-c), np.where(G > f32(c), f32(c), G))     # NaN stays NaN
        d = g + f32(wd) * P
        B = f32(mo) * B + d
        P = P + f32(-lr) * B
    return P.astype(f32), B.astype(f32)


SPECIALS = np.array([1.0, -1.0, np.inf, -np.inf, -0.0, np.nan, 1.0000001, -1.0000001, 0.99999994, 2.5, -7.0], f32)


class Model:
    """The tensors of the issue: numels around one 16-byte vector and around one chunk, several chunks plus a tail; a parameter that is a
    view one element into its storage with gradient and buffer at the same misalignment (scalar head + vector body), one whose
    gradient and buffer are aligned (scalar path), a frozen parameter and one whose .grad is None.  Host mirrors in P, B."""

    def __init__(self, O, seed, momentum=MO, weight_decay=WD, specials=True, **kw):
        C = O.CHUNK
        rng = np.random.default_rng(seed)
        self.rng, self.specials = rng, specials
        self.numels = [1, 3, 4, 5, C - 1, C, C + 1, 3 * C + 7]
        self.P = [(rng.standard_normal(n) * 0.1).astype(f32) for n in self.numels + [1031, 77, 10, 9]]
        self.P[7][4] = 0.0                                                                 # meets the gradient -0.0
        self.B = [np.zeros_like(p) for p in self.P]
        dev = torch.device("cuda")
        self.params = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p in self.P[:8]]
        self.i_shared, self.i_alone, self.i_frozen, self.i_nograd = 8, 9, 10, 11
        for i in (self.i_shared, self.i_alone):
            store = torch.zeros(self.P[i].size + 1, device=dev)
            store[1:].copy_(torch.from_numpy(self.P[i]))
            self.params.append(torch.nn.Parameter(store[1:]))
            assert self.params[-1].data_ptr() % 16 == 4 and self.params[-1].is_contiguous()
        self.params.append(torch.nn.Parameter(torch.from_numpy(self.P[self.i_frozen]).to(dev), requires_grad=False))
        self.params.append(torch.nn.Parameter(torch.from_numpy(self.P[self.i_nograd]).to(dev)))
        self.opt = O.FusedSGD(self.params, lr=lr_at(0), momentum=momentum, weight_decay=weight_decay, **kw)
        self.live = [i for i in range(len(self.params)) if i != self.i_frozen]
        for i in self.live:
            if i == self.i_nograd:
                continue
            if i == self.i_shared:
                self.params[i].grad = torch.zeros(self.P[i].size + 1, device=dev)[1:]
                self.opt.state[self.params[i]]["momentum_buffer"] = torch.zeros(self.P[i].size + 1, device=dev)[1:]
            else:
                self.params[i].grad = torch.zeros_like(self.params[i])
        self.G = None

    def draw(self, scale, specials=None):
        """new raw gradients on the host (None for the parameter that never gets one)"""
        G = [(self.rng.standard_normal(p.size) * scale).astype(f32) for p in self.P]
        if self.specials if specials is None else specials:
            for i in (4, 7, self.i_shared, self.i_alone):
                G[i][:SPECIALS.size] = SPECIALS                                            # head / vector body
                G[i][-SPECIALS.size:] = SPECIALS[::-1]                                     # tail
        G[self.i_nograd] = np.zeros_like(self.P[self.i_nograd])
        G[self.i_frozen] = None
        return G

    def write(self, G):
        """the gradients into the tensors the optimiser knows, in place"""
        for i in self.live:
            if i != self.i_nograd and G[i] is not None:
                self.params[i].grad.copy_(torch.from_numpy(G[i]))
        self.G = G

    def host_step(self, lr, loss=None, c=1.0, mo=MO, wd=WD):
        for i in self.live:
            self.P[i], self.B[i] = restate(self.P[i], self.G[i], self.B[i], lr, mo=mo, wd=wd, c=c, loss=loss)

    def check(self, what=""):
        torch.cuda.synchronize()
        for i, p in enumerate(self.params):
            assert same(p.detach().cpu().numpy(), self.P[i]), "%s parameter %d (%d elements)" % (what, i, self.P[i].size)
            if i == self.i_frozen:
                assert p.grad is None and p not in self.opt.state
                continue
            assert same(self.opt.state[p]["momentum_buffer"].cpu().numpy(), self.B[i]), "%s buffer %d" % (what, i)
            assert p.grad is not None and not bool(p.grad.any()), "%s gradient %d is not zero" % (what, i)
            assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), np.zeros(self.P[i].size, np.uint32))


@pytest.fixture
def variant(O):
    DEFAULTS = (O.GRID, O.NONTEMPORAL)

    def set_(grid, nt):
        O.GRID, O.NONTEMPORAL = grid, nt
    yield set_
    O.GRID, O.NONTEMPORAL = DEFAULTS


@pytest.mark.parametrize("grid,nt", [(0, 0), (3, 0), (0, 3), (0, 1)], ids=["plain", "three_workgroups", "nontemporal", "nontemporal_loads"])
def test_five_steps_are_the_float32_restatement_bit_for_bit(O, variant, grid, nt):
    variant(grid, nt)                                                                      # three workgroups: each loops over many tasks
    m = Model(O, seed=1)
    addresses = None
    for it in range(5):
        lr = lr_at(it)
        for group in m.opt.param_groups:
            group["lr"] = lr
        m.write(m.draw(3.0 if it % 2 else 0.3))
        m.opt.step()
        m.host_step(lr)
        m.check("step %d" % it)
        now = [(p.data_ptr(), p.grad.data_ptr()) for i, p in enumerate(m.params) if i != m.i_frozen]
        assert addresses is None or now == addresses                                       # nothing moves from step to step
        addresses = now
    assert m.opt.launches == 5 and m.opt.iteration() == 5                                  # one launch per step for the one group
    assert np.isnan(m.P[7][5]) and m.P[7][2] != m.P[7][3]                                  # the NaN went through, +-inf were clipped
    assert not np.array_equal(m.P[m.i_nograd], Model(O, seed=1).P[m.i_nograd])             # the zero gradient still decays the weights


def test_without_clip_and_without_momentum(O):
    m = Model(O, seed=2, momentum=0.0, weight_decay=0.0, specials=False, clip_value=None)
    for it in range(2):
        m.write(m.draw(3.0))
        m.opt.step()
        m.host_step(lr_at(0), c=None, mo=0.0, wd=0.0)
        m.check("step %d" % it)
    assert float(np.abs(m.B[7]).max()) > 1.5                                               # momentum 0: buf holds the unclipped gradient


def test_two_groups_one_launch_each_and_one_count(O):
    a = torch.nn.Parameter(torch.full((6,), 0.5, device="cuda"))
    b = torch.nn.Parameter(torch.full((9,), -0.25, device="cuda"))
    opt = O.FusedSGD([{"params": [a]}, {"params": [b], "lr": 0.5, "weight_decay": 0.0}], lr=0.1, momentum=MO, weight_decay=WD)
    a.grad, b.grad = torch.full_like(a, 0.75), torch.full_like(b, -3.0)
    opt.step()
    pa, ba = restate(np.full(6, 0.5, f32), np.full(6, 0.75, f32), np.zeros(6, f32), 0.1)
    pb, bb = restate(np.full(9, -0.25, f32), np.full(9, -3.0, f32), np.zeros(9, f32), 0.5, wd=0.0)
    assert same(a.detach().cpu().numpy(), pa) and same(b.detach().cpu().numpy(), pb)
    assert same(opt.state[b]["momentum_buffer"].cpu().numpy(), bb)
    assert opt.launches == 2 and opt.iteration() == 1                                      # only the last group's launch advances the counter


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_loss_backprop_within_twice_its_own_error(O):
    """golden = the reference's loss_backprop on the CPU (torch's SGD, which fuses a + alpha * b in its vector path); T = the same
    recurrence in float64 from the golden's inputs; E_ref = max |golden - T|, E = max |ours - T|; E <= 2 E_ref for parameters and buffers.
    Measured on the MI355X: see DESIGN.md 3.22."""
    z = H.golden()
    conf = H.conf_of(z, "train/conf")
    n, T = int(z["train/n_iter"]), int(z["train/n_tensors"])
    params = [torch.nn.Parameter(torch.from_numpy(z["train/init/%d" % k]).cuda()) for k in range(T)]
    opt = O.FusedSGD(params, lr=conf.lr, momentum=conf.momentum, weight_decay=conf.weight_decay)
    P64 = [z["train/init/%d" % k].astype(np.float64) for k in range(T)]
    B64 = [np.zeros_like(p) for p in P64]
    E = {"param": 0.0, "buf": 0.0}
    E_ref = {"param": 0.0, "buf": 0.0}
    before = None
    gated = 0
    for it in range(n):
        lr, loss = float(z["train/%d/lr" % it]), float(z["train/%d/loss" % it])
        assert np.float64(lr).view(np.uint64) == O.lr_schedule(conf)[it].view(np.uint64)
        O.adjust_lr(conf, opt, it)
        for k, p in enumerate(params):
            g = torch.from_numpy(z["train/%d/grad/%d" % (it, k)]).cuda()
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)
        opt.step(loss=torch.tensor(loss, dtype=torch.float32, device="cuda"))
        if loss > 0:
            for k in range(T):
                g = np.clip(z["train/%d/grad/%d" % (it, k)].astype(np.float64), -1.0, 1.0)
                B64[k] = conf.momentum * B64[k] + (g + conf.weight_decay * P64[k])
                P64[k] = P64[k] - lr * B64[k]
        ours = [(p.detach().cpu().numpy(), opt.state[p]["momentum_buffer"].cpu().numpy()) for p in params]
        for k in range(T):
            gp, gb = z["train/%d/param/%d" % (it, k)], z["train/%d/buf/%d" % (it, k)]
            E_ref["param"] = max(E_ref["param"], float(np.abs(gp.astype(np.float64) - P64[k]).max()))
            E_ref["buf"] = max(E_ref["buf"], float(np.abs(gb.astype(np.float64) - B64[k]).max()))
            E["param"] = max(E["param"], float(np.abs(ours[k][0].astype(np.float64) - P64[k]).max()))
            E["buf"] = max(E["buf"], float(np.abs(ours[k][1].astype(np.float64) - B64[k]).max()))
            assert not bool(params[k].grad.any())
        if not loss > 0:                                                                   # the gated iteration: bit for bit the previous state
            gated += 1
            assert all(same(o[0], b[0]) and same(o[1], b[1]) for o, b in zip(ours, before))
            assert all(same(z["train/%d/param/%d" % (it, k)], z["train/%d/param/%d" % (it - 1, k)]) for k in range(T))
        before = ours
    print("E_param %.4g E_ref_param %.4g E_buf %.4g E_ref_buf %.4g" % (E["param"], E_ref["param"], E["buf"], E_ref["buf"]))
    assert gated >= 1 and E_ref["param"] > 0 and E_ref["buf"] > 0
    assert E["param"] <= 2 * E_ref["param"], (E, E_ref)
    assert E["buf"] <= 2 * E_ref["buf"], (E, E_ref)


# ------------------------------------------------------------------------------------------------ the gate
def test_gate_is_applied_on_the_device(O):
    m = Model(O, seed=3)
    m.opt.set_iteration(7)
    done = 0
    for value in (0.0, -1.0, float("nan"), 1e-30, -0.0, float("inf")):
        m.write(m.draw(3.0))
        loss = torch.tensor(value, dtype=torch.float32, device="cuda")
        P0 = [p.copy() for p in m.P]
        m.opt.step(loss=loss)
        m.host_step(lr_at(0), loss=value)
        m.check("loss %r" % value)                                                         # also: every gradient is zero
        done += 1
        assert m.opt.iteration() == 7 + done                                               # the counter moves whether or not the update does
        moved = not all(same(a, b) for a, b in zip(P0, m.P))
        assert moved == (value > 0), value
    m.write(m.draw(0.3))
    m.opt.step(loss=torch.tensor([[2.0]], dtype=torch.float64, device="cuda"))            # any one-element tensor; float64 is converted on the device
    m.host_step(lr_at(0), loss=2.0)
    m.check("float64 loss")
    with pytest.raises(ValueError):
        m.opt.step(loss=torch.ones(2, device="cuda"))


# ------------------------------------------------------------------------------------------------ capturable
def test_captured_step_reads_schedule_loss_and_gradients_at_replay(O):
    table = np.array([lr_at(i) for i in range(6)], np.float64)
    cap = Model(O, seed=4, lr_table=table, capturable=True)
    eag = Model(O, seed=4)
    loss_dev = torch.zeros((), device="cuda")
    start = 1
    cap.opt.prepare()
    cap.opt.set_iteration(start)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.opt.step(loss=loss_dev)
    torch.cuda.synchronize()
    assert cap.opt.iteration() == start                                                    # captured, not run
    for i, value in enumerate((1.5, 0.0, 2.0, 0.25)):                                      # the second replay is gated and still counts
        G = cap.draw(3.0 if i % 2 else 0.3)
        cap.write(G)
        loss_dev.fill_(value)
        graph.replay()
        eag.write(G)
        for group in eag.opt.param_groups:
            group["lr"] = float(table[start + i])
        eag.opt.step(loss=torch.tensor(value, device="cuda"))
        eag.host_step(float(table[start + i]), loss=value)
        eag.check("eager %d" % i)
        cap.P, cap.B = eag.P, eag.B
        cap.check("replay %d" % i)
    assert cap.opt.iteration() == start + 4
    cap.opt.set_iteration(len(table) + 3)                                                  # past the end: the last entry
    G = cap.draw(0.3)
    cap.write(G)
    loss_dev.fill_(1.0)
    graph.replay()
    eag.G = G
    eag.host_step(float(table[-1]), loss=1.0)
    cap.P, cap.B = eag.P, eag.B
    cap.check("past the end")
    assert cap.opt.iteration() == len(table) + 4
    del graph


def test_backward_and_step_captured_together(O):
    """loss -> backward -> step(loss) as one graph: the gradients come from autograd inside the capture, the gate reads the captured loss"""
    table = np.array([lr_at(i) for i in range(8)], np.float64)

    def build(**kw):
        gen = torch.Generator().manual_seed(9)
        ps = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).cuda()) for n in (5, 1031, O.CHUNK + 1)]
        return ps, O.FusedSGD(ps, lr=lr_at(0), momentum=MO, weight_decay=WD, **kw)
    cp, copt = build(lr_table=table, capturable=True)
    ep, eopt = build()
    coeff = [torch.zeros_like(p) for p in cp]
    shift = torch.zeros((), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(10)
    values = (1.5, 0.25, 2.0, 0.0, 0.75)                                                    # the fourth step is gated

    def feed(i):
        for c in coeff:
            c.normal_(0, 2.0, generator=gen)
        shift.fill_(values[i])

    def whole(ps, opt):
        dot = sum((p * c).sum() for p, c in zip(ps, coeff))
        loss = dot - dot.detach() + shift                                                  # d loss / d p = coeff, value = shift
        loss.backward()
        opt.step(loss=loss)

    def eager(i):
        for group in eopt.param_groups:
            group["lr"] = float(table[i])
        whole(ep, eopt)

    def compare(what):
        torch.cuda.synchronize()
        for p, q in zip(cp, ep):
            assert same(p.detach().cpu().numpy(), q.detach().cpu().numpy()), what
            assert same(copt.state[p]["momentum_buffer"].cpu().numpy(), eopt.state[q]["momentum_buffer"].cpu().numpy()), what
            assert not bool(p.grad.any())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(2):                                                                 # warm-up on the capture stream, real steps
            feed(i)
            whole(cp, copt)
            eager(i)
    compare("warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            whole(cp, copt)
    torch.cuda.synchronize()
    start = [p.detach().clone() for p in cp]
    for i in range(2, 5):
        feed(i)
        graph.replay()
        eager(i)
        compare("replay %d" % i)
        if values[i] > 0:
            assert not all(torch.equal(a, p.detach()) for a, p in zip(start, cp))
        else:
            assert all(torch.equal(a, p.detach()) for a, p in zip(start, cp))
        start = [p.detach().clone() for p in cp]
    assert copt.iteration() == 5 and eopt.iteration() == 5
    del graph


# ------------------------------------------------------------------------------------------------ checkpoints
def test_state_dict_interchanges_with_torch_sgd(O):
    m = Model(O, seed=5, specials=False)
    for it in range(2):
        m.write(m.draw(3.0))
        m.opt.step()
        m.host_step(lr_at(0))
    m.check("two steps")
    saved = copy.deepcopy(m.opt.state_dict())                                              # what save_checkpoint would write
    live = [p for i, p in enumerate(m.params) if i != m.i_frozen]

    def clones():
        return [torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in m.params]
    # fused -> torch.optim.SGD
    tp = clones()
    sgd = torch.optim.SGD(tp, lr=1.0, momentum=0.1)
    sgd.load_state_dict(copy.deepcopy(saved))
    assert sgd.param_groups[0]["lr"] == lr_at(0) and sgd.param_groups[0]["momentum"] == MO
    # torch.optim.SGD -> fused, through torch's own state_dict
    fp = clones()
    back = O.FusedSGD(fp, lr=1.0, momentum=0.1)
    back.load_state_dict(copy.deepcopy(sgd.state_dict()))
    assert back.param_groups[0]["weight_decay"] == WD
    # a third step from all three
    G = m.draw(3.0)
    state2 = [(p.astype(np.float64), b.astype(np.float64)) for p, b in zip(m.P, m.B)]
    m.write(G)
    m.opt.step()
    m.host_step(lr_at(0))
    m.check("third step")
    for i, (q, r) in enumerate(zip(fp, tp)):
        if i != m.i_frozen:
            q.grad = torch.from_numpy(G[i]).cuda()
            r.grad = torch.from_numpy(G[i]).cuda()
    back.step()
    torch.nn.utils.clip_grad_value_(tp, 1)
    sgd.step()
    torch.cuda.synchronize()
    E = E_ref = 0.0
    for i, p in enumerate(m.params):
        assert same(fp[i].detach().cpu().numpy(), m.P[i]), i                                # the fused side: bit for bit
        if i == m.i_frozen:
            continue
        assert same(back.state[fp[i]]["momentum_buffer"].cpu().numpy(), m.B[i]), i
        P2, B2 = state2[i]
        B3 = MO * B2 + (np.clip(G[i].astype(np.float64), -1, 1) + WD * P2)
        P3 = P2 - lr_at(0) * B3
        for ours, theirs, T in ((m.P[i], tp[i].detach().cpu().numpy(), P3), (m.B[i], sgd.state[tp[i]]["momentum_buffer"].cpu().numpy(), B3)):
            E = max(E, float(np.abs(ours.astype(np.float64) - T).max()))
            E_ref = max(E_ref, float(np.abs(theirs.astype(np.float64) - T).max()))
    print("E %.4g E_ref %.4g" % (E, E_ref))
    assert E_ref > 0 and E <= 2 * E_ref, (E, E_ref)
    assert len(live) == len(saved["state"])


# ------------------------------------------------------------------------------------------------ the reference's call sequence
class Tiny(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


def test_reference_shaped_sequence_is_loss_backprop(O):
    C = O.CHUNK
    rng = np.random.default_rng(6)
    init = [torch.from_numpy((rng.standard_normal(n) * 0.1).astype(f32)).cuda() for n in (1, 5, C + 1, 1031)]
    coeff = [[torch.from_numpy((rng.standard_normal(t.numel()) * 3.0).astype(f32)).cuda() for t in init] for _ in range(3)]
    conf = H.AttrDict(solver_type="sgd", lr=0.004, momentum=MO, weight_decay=WD, lr_policy="poly", lr_steps=None, lr_target=0.004 * 1e-5, max_iter=50)
    nets = [Tiny(init), Tiny(init)]
    opts = [O.FusedSGD(n.parameters(), lr=conf.lr, momentum=conf.momentum, weight_decay=conf.weight_decay) for n in nets]

    def loss_of(net, it):
        dot = sum((p * c).sum() for p, c in zip(net.parameters(), coeff[it]))
        return dot - dot.detach() + 1.5
    addresses = None
    for it in range(3):
        # lib/core.py:99-113 as the reference has it, on a FusedSGD
        O.adjust_lr(conf, opts[0], it)
        loss = loss_of(nets[0], it)
        if loss > 0:
            loss.backward()
            torch.nn.utils.clip_grad_value_(nets[0].parameters(), 1)
            opts[0].step()
            launches = opts[0].launches
            opts[0].zero_grad()
            assert opts[0].launches == launches                                            # the step has zeroed them: nothing to launch
        now = [p.grad.data_ptr() for p in nets[0].parameters()]
        assert addresses is None or now == addresses
        addresses = now
        # and this module's
        O.adjust_lr(conf, opts[1], it)
        O.loss_backprop(loss_of(nets[1], it), nets[1], opts[1], conf=conf, iteration=it)
        torch.cuda.synchronize()
        for p, q in zip(nets[0].parameters(), nets[1].parameters()):
            assert same(p.detach().cpu().numpy(), q.detach().cpu().numpy())
            assert same(opts[0].state[p]["momentum_buffer"].cpu().numpy(), opts[1].state[q]["momentum_buffer"].cpu().numpy())
            assert not bool(p.grad.any()) and not bool(q.grad.any())
    assert not same(init[2].cpu().numpy(), list(nets[0].parameters())[2].detach().cpu().numpy())
    # a gradient written after the step is seen: zero_grad then does launch, and keeps the tensors
    loss_of(nets[0], 0).backward()
    launches = opts[0].launches
    opts[0].zero_grad()
    assert opts[0].launches == launches + 1 and [p.grad.data_ptr() for p in nets[0].parameters()] == addresses
    assert all(not bool(p.grad.any()) for p in nets[0].parameters())
    # conf or iteration missing: backward and the clip only (lib/core.py:109)
    before = [p.detach().clone() for p in nets[1].parameters()]
    O.loss_backprop(loss_of(nets[1], 1), nets[1], opts[1])
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, nets[1].parameters()))
    assert all(float(p.grad.abs().max()) <= 1.0 and bool(p.grad.any()) for p in nets[1].parameters())
