"""The yardstick of the DQN kernels (tests/dqn_grad_ref.py) held to account on the CPU, and the host-only parts of the feature: the
replay buffer, QNetworkMLP, DQNLearner's torch backend against a transcription of agents/dqn.py:84-112, the C calls' refusals."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import dqn_grad_ref as dr

MODES = pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
CASE = (257, 51, 100, 100)


def _case_id(c):
    return "B%d-F%d-H%d-%d" % c


@pytest.mark.parametrize("net", dr.NETS, ids=lambda n: "F%d-H%d-%d" % n)
def test_draw_is_exact_and_exercises_every_rule(net):
    """On the 257-row draw every case of the network is a prefix of: z1, z2 of both nets on both inputs bit-identical between fp64 and
    fp32 in two summation orders; each side of the Huber rule and its middle on >= 1 / 8 of the rows (both modes); each action taken
    on >= 1 / 4; each Q-value the target net's maximum on >= 1 / 8; the two nets' argmax on the next states apart on >= 1 / 16; no
    argmax of either net on the next states within twice the sum of its two logit bounds."""
    d = dr.inputs(dr.PARENT_ROWS, *net)
    for target in (False, True):
        for x in (d["x"], d["xn"]):
            n = dr._net(d, target, x)
            f64, f32, f32p = dr.forward(n, np.float64), dr.forward(n, np.float32), dr.forward(n, np.float32, perm=True)
            for k in ("z1", "z2"):
                assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f32[k], f32p[k]), k
        l = dr.forward(dr._net(d, target, d["xn"]), np.float64)["l"]
        E = dr.logit_bound(d, target, d["xn"])
        assert (np.abs(l[:, 0] - l[:, 1]) > 2 * (E[:, 0] + E[:, 1])).all()
    for double in (False, True):
        ref = dr.evaluate(d, double=double)
        delta = ref["q"] - ref["y"]
        shares = ((delta > 1).mean(), (delta < -1).mean(), (np.abs(delta) < 1).mean())
        assert min(shares) >= 1 / 8, shares
    assert 1 / 4 <= d["action"].mean() <= 3 / 4
    own = dr.evaluate(d, double=False)["next_action"]
    assert 1 / 8 <= own.mean() <= 7 / 8, own.mean()
    assert (own != dr.evaluate(d, double=True)["next_action"]).mean() >= 1 / 16


@MODES
def test_clamp_case_clamps_between_a_quarter_and_three_quarters(double):
    r = dr.reference(*CASE, double, "median")
    share = float((np.abs(r["ref"]["grad"]) == r["inputs"]["clamp"]).mean())
    assert 0.25 <= share <= 0.75, share


@MODES
def test_closed_form_equals_autograd_of_the_reference_expression(double):
    """fp64 autograd of agents/dqn.py:93-109 (DDQN: :128-135 with the per-row target) with nn.SmoothL1Loss and clamp_ on the same
    inputs gives the closed-form loss and clamped gradient (to fp64 rounding)."""
    r = dr.reference(*CASE, double, "median")
    d = r["inputs"]
    t64 = lambda k: torch.tensor(np.asarray(d[k], dtype=np.float64))  # noqa: E731

    def net(ps, x):
        h = torch.relu(x @ ps[0].t() + ps[1])
        h = torch.relu(h @ ps[2].t() + ps[3])
        return h @ ps[4].t() + ps[5]

    policy = [t64(k).requires_grad_() for k in dr.PARAM_NAMES]
    target = [t64(k) for k in dr.TARGET_NAMES]
    action, reward = torch.from_numpy(d["action"].copy()).view(-1, 1), t64("reward").view(-1, 1)
    q_values = net(policy, t64("x")).gather(1, action)
    with torch.no_grad():
        if double:
            next_action = net(policy, t64("xn")).argmax(dim=1, keepdim=True)
            next_q_values = net(target, t64("xn")).gather(1, next_action)
        else:
            next_q_values = net(target, t64("xn")).max(1)[0].unsqueeze(1)
    expected_q_values = reward + (next_q_values * dr.GAMMA)
    loss = torch.nn.SmoothL1Loss()(q_values, expected_q_values)
    loss.backward()
    for p in policy:
        p.grad.data.clamp_(-d["clamp"], d["clamp"])
    auto = np.concatenate([p.grad.numpy().reshape(-1) for p in policy])
    ref = r["ref"]
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-13
    assert np.abs(auto - ref["grad"]).max() < 1e-13
    assert np.abs(expected_q_values.numpy().reshape(-1) - ref["y"]).max() < 1e-13


@MODES
@pytest.mark.parametrize("case", dr.SWEEP, ids=_case_id)
def test_fp32_evaluations_stay_inside_the_bound(case, double):
    """An fp32 numpy evaluation of the formulas, in two summation orders, is inside the bound on every element of every output, with
    and without the clamp, and picks the same next actions."""
    for clamp in (np.inf, "median"):
        r = dr.reference(*case, double, clamp)
        for perm in (False, True):
            got = dr.evaluate(r["inputs"], np.float32, perm=perm, double=double)
            assert np.array_equal(got["next_action"], r["ref"]["next_action"])
            for k in r["bound"]:
                w = dr.worst(got[k], r["ref"][k], r["bound"][k])
                assert w <= 1.0, (clamp, perm, k, w)


@pytest.mark.parametrize("variant", dr.VARIANTS)
def test_wrong_variants_leave_the_bound(variant):
    """Each wrong variant is outside the bound on more than half of the elements of at least one parameter's gradient; `no_clamp`,
    which can only differ where the clamp acts, on every element the median clamp reaches (at least a quarter of them)."""
    double = variant == "dqn_for_ddqn"
    r = dr.reference(*CASE, double, "median" if variant == "no_clamp" else np.inf)
    got = dr.evaluate(r["inputs"], np.float32, variant=variant, double=double)
    ratio = dr.ratio_to_bound(got["grad"], r["ref"]["grad"], r["bound"]["grad"])
    if variant == "no_clamp":
        reached = np.abs(r["ref"]["grad"]) == r["inputs"]["clamp"]
        assert reached.mean() >= 0.25 and (ratio[reached] > 1).mean() > 0.99
        return
    fractions = {n: float((ratio[s] > 1).mean()) for n, s in dr.param_slices(*CASE[1:], 2).items()}
    assert max(fractions.values()) > 0.5, fractions


# ---- the replay buffer

def _rows(lo, hi, F=3):
    i = torch.arange(lo, hi, dtype=torch.float32)
    return i[:, None] + torch.arange(F) / 10.0, (torch.arange(lo, hi) % 2), -i, i[:, None] + 0.5 + torch.arange(F) / 10.0


def test_replay_buffer_equals_a_deque_across_the_wrap():
    from mdr_amd.dqn import DeviceReplayBuffer
    buf, ref = DeviceReplayBuffer(10, 3, "cpu"), collections.deque(maxlen=10)
    lo = 0
    for n in (4, 3, 5, 1, 7, 10, 2):      # uneven pushes, several wraps, one of exactly the capacity
        s, a, r, sn = _rows(lo, lo + n)
        buf.push(s, a, r, sn)
        ref.extend(range(lo, lo + n))
        lo += n
        assert len(buf) == len(ref)
        order = buf.chronological()
        want = _rows(0, lo)
        for got, w in zip((buf.state, buf.action, buf.reward, buf.next_state), want):
            assert torch.equal(got[order], w[list(ref)])
    assert buf.action.dtype == torch.int64 and buf.state.shape == (10, 3)


def test_replay_buffer_keeps_the_tail_of_an_oversize_push():
    from mdr_amd.dqn import DeviceReplayBuffer
    buf = DeviceReplayBuffer(8, 3, "cpu")
    buf.push(*_rows(0, 3))
    buf.push(*_rows(3, 24))      # 21 rows into 8
    assert len(buf) == 8
    assert torch.equal(buf.reward[buf.chronological()], -torch.arange(16, 24, dtype=torch.float32))
    buf.push(*_rows(24, 26))
    assert torch.equal(buf.reward[buf.chronological()], -torch.arange(18, 26, dtype=torch.float32))
    with pytest.raises(ValueError):
        buf.push(torch.zeros((2, 4)), torch.zeros(2), torch.zeros(2), torch.zeros((2, 4)))


def test_replay_buffer_takes_the_dict_of_collect_dqn_transitions():
    from mdr_amd.dqn import DeviceReplayBuffer
    T, A, F = 3, 4, 5
    state = torch.arange((T + 1) * A * F, dtype=torch.float32).view(T + 1, A, F)
    batch = dict(state=state, action=torch.arange(T * A).view(T, A) % 2, reward=torch.arange(T * A, dtype=torch.float32).view(T, A))
    buf = DeviceReplayBuffer(32, F, "cpu")
    buf.push_batch(batch)
    assert len(buf) == T * A
    assert torch.equal(buf.state[:T * A], state[:T].reshape(-1, F)) and torch.equal(buf.next_state[:T * A], state[1:].reshape(-1, F))
    assert torch.equal(buf.reward[:T * A], torch.arange(T * A, dtype=torch.float32))      # (t, agent) order


def test_replay_buffer_samples_the_filled_part_reproducibly():
    from mdr_amd.dqn import DeviceReplayBuffer
    buf = DeviceReplayBuffer(100, 3, "cpu")
    with pytest.raises(ValueError):
        buf.sample(4)
    buf.push(*_rows(0, 7))
    draw = lambda seed: buf.sample(1000, torch.Generator().manual_seed(seed))  # noqa: E731
    a = draw(1)
    assert a.dtype == torch.int64 and a.shape == (1000,) and int(a.min()) == 0 and int(a.max()) == 6      # inside [0, len), every slot, repeats
    assert torch.equal(a, draw(1)) and not torch.equal(a, draw(2))


# ---- the modules and the learner

def test_qnetwork_loads_the_reference_keys_and_returns_raw_values():
    import mdr_amd
    from mdr_amd.dqn import QNetworkMLP
    g = torch.Generator().manual_seed(0)
    shapes = {"fc.0.weight": (100, 22), "fc.0.bias": (100,), "fc.1.weight": (100, 100), "fc.1.bias": (100,), "fc.2.weight": (2, 100), "fc.2.bias": (2,)}
    sd = {k: torch.randn(s, generator=g) * 0.2 for k, s in shapes.items()}      # the keys of DQN.save()'s actor.pth (DQN_network)
    net = QNetworkMLP(22)
    net.load_state_dict(sd)
    assert list(net.state_dict().keys()) == list(shapes)
    x = torch.randn((9, 22), generator=g)
    h = torch.relu(x @ sd["fc.0.weight"].t() + sd["fc.0.bias"])
    h = torch.relu(h @ sd["fc.1.weight"].t() + sd["fc.1.bias"])
    want = h @ sd["fc.2.weight"].t() + sd["fc.2.bias"]
    got = net(x)
    assert torch.allclose(got, want, rtol=0, atol=1e-6) and bool((got < 0).any())      # no softmax: raw Q-values
    assert mdr_amd.QNetworkMLP is QNetworkMLP and mdr_amd.dqn.DQNLearner is mdr_amd.DQNLearner
    # the rollout code reads `fc` only
    assert [type(m) for m in net.fc] == [torch.nn.Linear] * 3 and not hasattr(net, "softmax")


def _filled_learner(double, tau, **kw):
    from mdr_amd.dqn import DQNLearner, QNetworkMLP
    torch.manual_seed(5)
    net = QNetworkMLP(6, layers=(16, 16))
    learner = DQNLearner(net, 1e-2, gamma=0.9, tau=tau, buffer_capacity=64, batch_size=32, double=double, backend="torch", **kw)
    g = torch.Generator().manual_seed(6)
    n = 50
    learner.buffer.push(torch.randn((n, 6), generator=g), torch.randint(0, 2, (n,), generator=g), 3 * torch.randn(n, generator=g),
                        torch.randn((n, 6), generator=g))
    return learner


@MODES
def test_torch_backend_performs_the_reference_update(double):
    """One DQNLearner.update(backend="torch") on CPU tensors against agents/dqn.py:88-112 written out (DDQN: the per-row target):
    the same policy parameters bit for bit, every target parameter within 3 u ((1 - tau) |t| + tau |p|) of the fp64 blend."""
    from mdr_amd.dqn import QNetworkMLP
    tau = 0.01
    learner = _filled_learner(double, tau)
    with torch.no_grad():      # a target net of its own, so that the two modes differ
        for p in learner.target_net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(7)))
    policy_net, target_net = QNetworkMLP(6, layers=(16, 16)), QNetworkMLP(6, layers=(16, 16))
    policy_net.load_state_dict(learner.policy_net.state_dict())
    target_net.load_state_dict(learner.target_net.state_dict())
    optimizer = torch.optim.Adam(policy_net.parameters(), 1e-2)
    index = learner.sample(3)
    buf = learner.buffer
    state, action, reward, next_state = buf.state[index], buf.action[index].view(-1, 1), buf.reward[index].view(-1, 1), buf.next_state[index]
    q_values = policy_net(state).gather(1, action)
    if double:
        next_action = policy_net(next_state).argmax(dim=1, keepdim=True)
        next_q_values = target_net(next_state).gather(1, next_action).detach()
    else:
        next_q_values = target_net(next_state).max(1)[0].detach().unsqueeze(1)
    expected_q_values = reward + (next_q_values * 0.9)
    loss = torch.nn.SmoothL1Loss()(q_values, expected_q_values)
    optimizer.zero_grad()
    loss.backward()
    for param in policy_net.parameters():
        param.grad.data.clamp_(-1, 1)
    optimizer.step()
    old_target = [p.detach().double().clone() for p in learner.target_net.parameters()]
    seen = []
    learner.before_step = lambda lrn: seen.append([p.grad.clone() for p in lrn.policy_net.parameters()])
    got = learner.update(seed=3)
    assert got.dim() == 0 and float(got) == float(loss.detach()) and learner.training_step == 1 and len(seen) == 1
    assert all(float(g.abs().max()) <= 1.0 for g in seen[0])
    for p, q in zip(learner.policy_net.parameters(), policy_net.parameters()):
        assert torch.equal(p, q)
    U = 2.0 ** -24
    for t, t0, p in zip(learner.target_net.parameters(), old_target, policy_net.parameters()):
        p64 = p.detach().double()
        assert bool(((t.detach().double() - ((1 - tau) * t0 + tau * p64)).abs() <= 3 * U * ((1 - tau) * t0.abs() + tau * p64.abs())).all())


def test_learner_waits_for_a_minibatch_and_reads_the_config():
    from mdr_amd.dqn import DQNLearner, QNetworkMLP
    net = QNetworkMLP(6, layers=(16, 16))
    prop = {"network_layers": [16, 16], "gamma": 0.99, "tau": 0.01, "buffer_capacity": 128, "lr": 1e-3, "batch_size": 256,
            "epsilon_decay": 0.99998, "min_epsilon": 0.01}
    learner = DQNLearner.from_config(prop, net, double=True, backend="torch")
    assert (learner.gamma, learner.tau, learner.batch_size, learner.buffer.capacity, learner.double) == (0.99, 0.01, 256, 128, True)
    assert all(torch.equal(p, q) for p, q in zip(learner.target_net.parameters(), net.parameters()))      # agents/dqn.py:35
    learner.buffer.push(torch.zeros((100, 6)), torch.zeros(100, dtype=torch.int64), torch.zeros(100), torch.zeros((100, 6)))
    assert learner.update() is None and learner.training_step == 0      # agents/dqn.py:85-86
    assert not learner.uses_kernels(256)                                # CPU parameters: auto falls back to torch
    with pytest.raises(ValueError, match="backend"):
        DQNLearner(net, 1e-3, buffer_capacity=8, backend="cuda")
    with pytest.raises(ValueError, match="backend='hip'"):
        DQNLearner(net, 1e-3, buffer_capacity=8, backend="hip")
    still = _filled_learner(True, 0.5, soft_update=False)               # the reference's DDQN never blends its target net
    before = [p.detach().clone() for p in still.target_net.parameters()]
    assert still.update() is not None
    assert all(torch.equal(p, q) for p, q in zip(still.target_net.parameters(), before))


# ---- the C calls' host-side refusals: nothing below reaches a device

def _mlp(F=51, H1=100, H2=100, O=2, size=None, ptr=0x1000):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, F, H1, H2, O, *([ptr] * 6))


def test_signatures_match_the_header():
    lib = nat.load()
    assert len(lib.mdr_dqn_target.argtypes) == 13 and len(lib.mdr_dqn_grad.argtypes) == 14
    assert lib.mdr_dqn_target.argtypes[7] is C.c_float and lib.mdr_dqn_grad.argtypes[7] is C.c_float
    assert nat.MDR_ABI_VERSION == 5 and lib.mdr_abi_version() == 5


def test_target_call_refuses_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
    net, pol = _mlp(), _mlp()

    def call(target=net, policy=None, ns=p, ld=51, B=16, reward=p, gamma=0.99, mw=0, y=p, na=p):
        return lib.mdr_dqn_target(C.byref(target) if target is not None else None, C.byref(policy) if policy is not None else None, ns, ld,
                                  None, B, reward, C.c_float(gamma), mw, y, None, na, None)

    for kw in (dict(target=None), dict(ns=None), dict(reward=None), dict(y=None), dict(ld=50), dict(B=-1), dict(mw=-1), dict(gamma=float("nan")),
               dict(gamma=float("inf")), dict(target=_mlp(size=8)), dict(target=_mlp(ptr=None)), dict(policy=pol, na=None),
               dict(policy=_mlp(size=8)), dict(policy=_mlp(ptr=None))):
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(target=_mlp(F=65), ld=128), dict(target=_mlp(H1=129)), dict(target=_mlp(H2=129)), dict(target=_mlp(O=1)), dict(target=_mlp(O=3)),
               dict(policy=_mlp(F=50)), dict(policy=_mlp(H1=96)), dict(policy=_mlp(H2=96)), dict(policy=_mlp(O=1))):
        assert call(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert call(B=0) == nat.MDR_OK and call(B=0, policy=pol) == nat.MDR_OK      # zero rows: nothing to launch


def test_gradient_call_refuses_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    net = _mlp()

    def call(net=net, state=p, ld=51, B=16, action=p, y=p, clamp=1.0, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_dqn_grad(C.byref(net) if net is not None else None, state, ld, None, B, action, y, C.c_float(clamp), mw, ws, grad, loss,
                                None, None)

    for kw in (dict(net=None), dict(state=None), dict(action=None), dict(y=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ld=50),
               dict(B=-1), dict(mw=-1), dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(ws=C.c_void_p(0x1004)),
               dict(net=_mlp(size=8)), dict(net=_mlp(ptr=None))):
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(net=_mlp(F=65), ld=128), dict(net=_mlp(H1=129)), dict(net=_mlp(H2=129)), dict(net=_mlp(O=1)), dict(net=_mlp(O=3))):
        assert call(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert lib.mdr_mlp_grad_floats(C.byref(net)) == 100 * 51 + 100 + 100 * 100 + 100 + 2 * 100 + 2      # serves mdr_dqn_grad unchanged
