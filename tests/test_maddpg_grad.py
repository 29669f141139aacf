"""MADDPG's update step on the CPU: tests/maddpg_grad_ref.py held to account (its closed forms against autograd of the reference's
expressions in fp64, its bound against fp32 evaluations in several summation orders and against deliberately wrong variants), the
joint replay buffer, DDPGNetworkMLP, the torch backend of MADDPGLearner against agents/ddpg.py:305-339 written out, and the host-side
refusals of mdr_maddpg_target / mdr_maddpg_critic_grad / mdr_maddpg_actor_grad.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mdr_amd import _native as nat
from tests import maddpg_grad_ref as R

SMALL = [net for net in R.NETS if net[0] < 20]


def _torch_net(d, prefix, dtype=torch.float64):
    p = [torch.tensor(np.asarray(d[prefix + n]), dtype=dtype, requires_grad=True) for n in R.PARAM_NAMES]

    def f(x):
        return F.relu(F.relu(x @ p[0].T + p[1]) @ p[2].T + p[3]) @ p[4].T + p[5]

    return p, f


def _hard(logits, noise, tau):
    """F.gumbel_softmax(hard=True) with the given gumbel noise."""
    y_soft = ((logits + noise) / tau).softmax(-1)
    y_hard = torch.zeros_like(logits).scatter_(-1, y_soft.max(-1, keepdim=True)[1], 1.0)
    return y_hard - y_soft.detach() + y_soft


@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_draw_leaves_no_pick_to_rounding(net):
    d = R.draw(*net)      # asserts it itself after at most four passes
    for tau in (1.0, 0.5):
        assert not any(b.any() for b in R._pick_bad(d, tau))
    if net[0] > 1:
        na = R.evaluate(R.inputs(65, *net), 0)["next_action"]
        assert 0.1 < na.mean() < 0.9      # both actions are picked


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("net,agent", [(SMALL[0], 0), (SMALL[1], 1), (SMALL[2], 1), (SMALL[3], 4)], ids=str)
def test_closed_forms_equal_autograd_of_the_reference_expressions(net, agent, tau):
    """ddpg.py:312-339 on fp64 tensors with hard - soft.detach() + soft on the drawn noise, against evaluate()."""
    N = net[0]
    B = 33
    d = R.inputs(B, *net)
    ref = R.evaluate(d, agent, tau)
    t64 = lambda k: torch.tensor(np.asarray(d[k]), dtype=torch.float64)      # noqa: E731
    state, next_state = t64("state"), t64("next_state")
    action = F.one_hot(torch.tensor(d["action"]), 2).double()
    (_, tgt_actor), (_, tgt_critic) = _torch_net(d, "t"), _torch_net(d, "tc")
    (ap, actor), (cp, critic) = _torch_net(d, ""), _torch_net(d, "c")
    with torch.no_grad():
        next_action = _hard(tgt_actor(next_state), t64("noise_t"), tau)
        next_q = tgt_critic(torch.cat((next_state.reshape(B, -1), next_action.reshape(B, -1)), 1)).squeeze(1)
        y = t64("reward")[:, agent] + R.GAMMA * next_q
    assert np.array_equal(next_action[:, :, 1].numpy().astype(np.uint8), ref["next_action"])
    np.testing.assert_allclose(y.numpy(), ref["y"], rtol=1e-12, atol=1e-12)
    q = critic(torch.cat((state.reshape(B, -1), action.reshape(B, -1)), 1)).squeeze(1)
    closs = F.mse_loss(q, y)
    closs.backward()
    np.testing.assert_allclose(float(closs.detach()), ref["closs"], rtol=1e-12)
    np.testing.assert_allclose(np.concatenate([p.grad.numpy().reshape(-1) for p in cp]), ref["cgrad"], rtol=1e-9, atol=1e-13)
    for p in cp:
        p.grad = None
    logits = actor(state[:, agent])
    own = _hard(logits, t64("noise_a")[:, agent], tau)
    joint = torch.cat((action[:, :agent], own[:, None], action[:, agent + 1:]), 1)
    Q = critic(torch.cat((state.reshape(B, -1), joint.reshape(B, -1)), 1)).squeeze(1)
    aloss = -Q.mean() + R.PSE * logits.pow(2).mean()
    aloss.backward()
    np.testing.assert_allclose(Q.detach().numpy(), ref["Q"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(float(aloss.detach()), ref["aloss"], rtol=1e-12)
    np.testing.assert_allclose(np.concatenate([p.grad.numpy().reshape(-1) for p in ap]), ref["agrad"], rtol=1e-9, atol=1e-14)
    assert N == action.shape[1]


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_fp32_evaluations_stay_inside_the_bound(net, tau):
    B = 33 if net[0] == 20 else 65
    agent = net[0] // 2
    case = R.reference(B, *net, agent, tau)
    for perm in (False, True):
        got = R.evaluate(case["inputs"], agent, tau, dtype=np.float32, perm=perm)
        assert np.array_equal(got["next_action"], case["ref"]["next_action"])
        for k in R.FLOAT_KEYS:
            assert R.worst(got[k], case["ref"][k], case["bound"][k]) <= 1.0, (k, perm)
    # torch's fp32 autograd order as a third: the target and the critic's step
    d = case["inputs"]
    (cp, critic) = _torch_net(d, "c", torch.float32)
    x = torch.tensor(R.joint(d["state"], d["action"]))
    q = critic(x).squeeze(1)
    F.mse_loss(q, torch.tensor(case["ref"]["y"].astype(np.float32))).backward()
    got = np.concatenate([p.grad.numpy().reshape(-1) for p in cp])
    assert R.worst(got, case["ref"]["cgrad"], case["bound"]["cgrad"]) <= 1.0


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_variants_leave_the_bound(variant):
    agent, tau = 1, 0.5
    case = R.reference(65, *SMALL[2], agent, tau)
    got = R.evaluate(case["inputs"], agent, tau, variant=variant)
    assert R.worst_of(got, case["ref"], case["bound"]) > 1.0


# ---- the buffer

def _steps(n, N=3, F_len=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, N, F_len), generator=g), torch.randint(0, 2, (n, N), generator=g), torch.randn((n, N), generator=g),
            torch.randn((n, N, F_len), generator=g))


def test_joint_buffer_is_a_ring_across_the_wrap_and_keeps_the_tail_of_an_oversize_push():
    from mdr_amd.maddpg import JointReplayBuffer
    buf = JointReplayBuffer(10, 3, 4, "cpu")
    s, a, r, ns = _steps(27)
    for lo, hi in ((0, 4), (4, 9), (9, 16), (16, 27)):      # the third push wraps, the fourth is larger than the ring
        buf.push(s[lo:hi], a[lo:hi], r[lo:hi], ns[lo:hi])
        idx = buf.chronological()
        kept = slice(max(hi - 10, 0), hi)
        assert len(buf) == min(hi, 10)
        assert torch.equal(buf.state[idx], s[kept]) and torch.equal(buf.action[idx], a[kept])
        assert torch.equal(buf.reward[idx], r[kept]) and torch.equal(buf.next_state[idx], ns[kept])
    with pytest.raises(ValueError):
        buf.push(s[:2, :2], a[:2], r[:2], ns[:2])


def test_joint_buffer_samples_without_replacement_and_reproducibly():
    from mdr_amd.maddpg import JointReplayBuffer
    buf = JointReplayBuffer(64, 3, 4, "cpu")
    buf.push(*_steps(20))
    a = buf.sample(20, torch.Generator().manual_seed(4))
    b = buf.sample(20, torch.Generator().manual_seed(4))
    assert torch.equal(a, b) and sorted(a.tolist()) == list(range(20))      # every stored env-step once: no replacement
    assert len(set(buf.sample(7, torch.Generator().manual_seed(5)).tolist())) == 7
    with pytest.raises(ValueError):
        buf.sample(21)


def test_joint_buffer_takes_the_dict_of_collect_maddpg_transitions():
    from mdr_amd.maddpg import JointReplayBuffer
    T, E, N, F_len = 3, 2, 3, 4
    g = torch.Generator().manual_seed(1)
    batch = {"state": torch.randn((T + 1, E, N, F_len), generator=g), "action": torch.randint(0, 2, (T, E, N), generator=g),
             "reward": torch.randn((T, E, N), generator=g)}
    buf = JointReplayBuffer(16, N, F_len, "cpu")
    buf.push_batch(batch)
    assert len(buf) == T * E
    assert torch.equal(buf.state[:6], batch["state"][:T].reshape(6, N, F_len))
    assert torch.equal(buf.next_state[:6], batch["state"][1:].reshape(6, N, F_len))
    assert torch.equal(buf.action[:6], batch["action"].reshape(6, N)) and torch.equal(buf.reward[:6], batch["reward"].reshape(6, N))


# ---- the network and the learner

def test_ddpg_network_loads_the_reference_keys_and_follows_its_initialisation():
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(0)
    net = DDPGNetworkMLP(7, 2, 12)
    assert list(net.state_dict()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"]
    ref = torch.nn.Sequential(torch.nn.Linear(7, 12), torch.nn.ReLU(), torch.nn.Linear(12, 12), torch.nn.ReLU(), torch.nn.Linear(12, 2))
    net.load_state_dict({"net." + k: v for k, v in ref.state_dict().items()})
    x = torch.randn(5, 7)
    assert torch.equal(net(x), ref(x))
    fresh = DDPGNetworkMLP(7, 2, 12)
    gain = torch.nn.init.calculate_gain("relu")
    for lin in fresh.fc:      # network.py:94-100: xavier_uniform_ with the ReLU gain, biases 0.01
        assert bool((lin.bias == 0.01).all())
        limit = gain * (6.0 / (lin.in_features + lin.out_features)) ** 0.5
        top = float(lin.weight.detach().abs().max())
        assert 0.5 * limit < top <= limit


def _filled_learner(N=2, F_len=5, H=16, B=8, **kw):
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
    torch.manual_seed(5)
    actor, critic = DDPGNetworkMLP(F_len, 2, H), DDPGNetworkMLP(N * (F_len + 2), 1, H)
    learner = MADDPGLearner(actor, critic, N, 1e-2, 3e-2, gamma=0.9, soft_tau=0.05, gumbel_tau=0.5, batch_size=B, buffer_capacity=32,
                            backend="torch", **kw)
    learner.buffer.push(*_steps(20, N, F_len, seed=6))
    return learner


def test_torch_backend_performs_the_reference_update():
    """One MADDPGLearner.update(backend="torch") on CPU tensors against ddpg.py:305-339 and :167-174 written out for two agents: the
    same actor and critic bit for bit, every target parameter within 3 u of the fp64 blend."""
    import copy
    learner = _filled_learner()
    N, B = 2, 8
    with torch.no_grad():      # targets of their own
        for p in list(learner.tgt_actor.parameters()) + list(learner.tgt_critic.parameters()):
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(7)))
    actor, critic = copy.deepcopy(learner.actor), copy.deepcopy(learner.critic)
    tgt_actor, tgt_critic = copy.deepcopy(learner.tgt_actor), copy.deepcopy(learner.tgt_critic)
    a_opt, c_opt = torch.optim.Adam(actor.parameters(), 1e-2), torch.optim.Adam(critic.parameters(), 3e-2)
    index, noise_t, noise_a = learner.draws(3)
    assert index.shape == (N, B) and noise_t.shape == (N, B, N, 2) and noise_a.shape == (N, B, 2)
    assert all(len(set(row.tolist())) == B for row in index)
    buf = learner.buffer
    a_losses, c_losses = [], []
    for a in range(N):
        idx = index[a]
        state = [buf.state[idx][:, k] for k in range(N)]
        act = [F.one_hot(buf.action[idx][:, k], 2).float() for k in range(N)]
        next_state = [buf.next_state[idx][:, k] for k in range(N)]
        next_act = [_hard(tgt_actor(next_state[k]), noise_t[a][:, k], 0.5).detach() for k in range(N)]
        critic_value = critic(torch.cat(state + act, 1)).squeeze(1)
        next_value = tgt_critic(torch.cat(next_state + next_act, 1)).squeeze(1)
        target_value = buf.reward[idx][:, a] + 0.9 * next_value
        critic_loss = F.mse_loss(critic_value, target_value.detach(), reduction="mean")
        c_opt.zero_grad()
        critic_loss.backward()
        torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5)
        c_opt.step()
        logits = actor(state[a])
        act[a] = _hard(logits, noise_a[a], 0.5)
        actor_loss = -critic(torch.cat(state + act, 1)).squeeze(1).mean() + 1e-3 * torch.pow(logits, 2).mean()
        a_opt.zero_grad()
        actor_loss.backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 0.5)
        a_opt.step()
        a_losses.append(actor_loss.detach())
        c_losses.append(critic_loss.detach())
    old = [p.detach().double().clone() for p in list(learner.tgt_actor.parameters()) + list(learner.tgt_critic.parameters())]
    got = learner.update(seed=3)
    assert learner.training_step == 1 and got[0].shape == (N,) and got[1].shape == (N,)
    assert torch.equal(got[0], torch.stack(a_losses)) and torch.equal(got[1], torch.stack(c_losses))
    for p, q in zip(list(learner.actor.parameters()) + list(learner.critic.parameters()), list(actor.parameters()) + list(critic.parameters())):
        assert torch.equal(p, q)
    U = 2.0 ** -24
    new = list(actor.parameters()) + list(critic.parameters())
    for t, t0, p in zip(list(learner.tgt_actor.parameters()) + list(learner.tgt_critic.parameters()), old, new):
        p64 = p.detach().double()
        assert bool(((t.detach().double() - (0.95 * t0 + 0.05 * p64)).abs() <= 3 * U * (0.95 * t0.abs() + 0.05 * p64.abs())).all())


def test_learner_waits_for_a_minibatch_and_reads_the_config():
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner, supported
    prop = {"actor_hidden_dim": 16, "critic_hidden_dim": 16, "gamma": 0.99, "lr_critic": 3e-3, "lr_actor": 1e-3, "soft_tau": 0.01,
            "clip_param": 0.2, "max_grad_norm": 0.5, "ddpg_update_time": 10, "batch_size": 64, "buffer_capacity": 128, "episode_num": 10000,
            "learn_interval": 100, "random_steps": 100, "gumbel_softmax_tau": 1, "DDPG_shared": True}
    actor, critic = DDPGNetworkMLP(5, 2, 16), DDPGNetworkMLP(2 * 7, 1, 16)
    learner = MADDPGLearner.from_config(prop, actor, critic, 2, backend="torch")
    assert (learner.gamma, learner.soft_tau, learner.gumbel_tau, learner.batch_size, learner.buffer.capacity) == (0.99, 0.01, 1.0, 64, 128)
    assert learner.actor_optimizer.param_groups[0]["lr"] == 1e-3 and learner.critic_optimizer.param_groups[0]["lr"] == 3e-3
    assert all(torch.equal(p, q) for p, q in zip(learner.tgt_actor.parameters(), actor.parameters()))      # ddpg.py:79-91
    assert all(torch.equal(p, q) for p, q in zip(learner.tgt_critic.parameters(), critic.parameters()))
    learner.buffer.push(*_steps(20, 2, 5))
    assert learner.update() is None and learner.training_step == 0
    assert not learner.uses_kernels(64) and not supported(actor, critic, 2)      # CPU parameters: auto falls back to torch
    with pytest.raises(ValueError, match="backend"):
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=8, backend="cuda")
    with pytest.raises(ValueError, match="backend='hip'"):
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=8, backend="hip")
    with pytest.raises(ValueError, match="nb_agents"):
        MADDPGLearner(actor, critic, 3, 1e-3, 1e-3, buffer_capacity=8, backend="torch")


# ---- the C calls' host-side refusals and size functions: nothing below reaches a device

def _mlp(K=51, H1=256, H2=256, O=2, size=None, ptr=0x1000):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, K, H1, H2, O, *([ptr] * 6))


def test_signatures_match_the_header():
    lib = nat.load()
    assert len(lib.mdr_maddpg_target.argtypes) == 17 and len(lib.mdr_maddpg_critic_grad.argtypes) == 14
    assert len(lib.mdr_maddpg_actor_grad.argtypes) == 19
    assert lib.mdr_maddpg_target.argtypes[10] is C.c_float and lib.mdr_maddpg_target.argtypes[11] is C.c_float
    assert lib.mdr_maddpg_actor_grad.argtypes[10] is C.c_float and lib.mdr_maddpg_actor_grad.argtypes[11] is C.c_float


def test_size_functions():
    lib = nat.load()
    actor, critic = _mlp(), _mlp(K=20 * 53, O=1)
    assert lib.mdr_maddpg_grad_floats(C.byref(actor)) == 256 * 51 + 256 + 256 * 256 + 256 + 2 * 256 + 2
    assert lib.mdr_maddpg_grad_floats(C.byref(critic)) == 256 * 1060 + 256 + 256 * 256 + 256 + 256 + 1
    odd = _mlp(K=63, H1=97, H2=113)
    assert lib.mdr_maddpg_grad_floats(C.byref(odd)) == 97 * 63 + 97 + 113 * 97 + 113 + 2 * 113 + 2
    for bad in (_mlp(K=1281, O=1), _mlp(H1=257), _mlp(H2=257), _mlp(O=3), _mlp(size=8), _mlp(K=0)):
        assert lib.mdr_maddpg_grad_floats(C.byref(bad)) == -1
    # rows padded to 16: h1, dz1, h2, dz2 [Bp][256] each, dlogits [Bp][2], the loss terms [Bp]
    assert lib.mdr_maddpg_workspace_bytes(C.byref(actor), C.byref(critic), 20, 64, 0) == 64 * (4 * 256 + 3) * 4
    assert lib.mdr_maddpg_workspace_bytes(C.byref(actor), C.byref(critic), 20, 65, 2) == 80 * (4 * 256 + 3) * 4
    wide = lib.mdr_maddpg_workspace_bytes(C.byref(_mlp(K=63, H1=97, H2=113)), C.byref(_mlp(K=5 * 65, H1=30, H2=20, O=1)), 5, 17, 0)
    assert wide == 32 * (2 * 112 + 2 * 128 + 3) * 4      # the larger of the two nets' needs
    assert lib.mdr_maddpg_workspace_bytes(C.byref(actor), C.byref(critic), 20, 0, 0) >= 16
    for kw in (dict(N=19), dict(B=-1), dict(mw=-1), dict(a=_mlp(K=65), c=_mlp(K=20 * 67, O=1)), dict(c=_mlp(K=1060, H1=257, O=1)), dict(a=None)):
        a, c = kw.get("a", actor), kw.get("c", critic)
        assert lib.mdr_maddpg_workspace_bytes(C.byref(a) if a is not None else None, C.byref(c), kw.get("N", 20), kw.get("B", 64),
                                              kw.get("mw", 0)) == -1, kw


def test_target_call_refuses_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
    actor, critic = _mlp(), _mlp(K=20 * 53, O=1)

    def call(a=actor, c=critic, ns=p, ld=1020, reward=p, B=16, N=20, agent=3, noise=p, tau=1.0, gamma=0.99, mw=0, y=p, na=p):
        return lib.mdr_maddpg_target(C.byref(a) if a is not None else None, C.byref(c) if c is not None else None, ns, ld, reward, None, B, N,
                                     agent, noise, C.c_float(tau), C.c_float(gamma), mw, y, None, na, None)

    for kw in (dict(a=None), dict(c=None), dict(ns=None), dict(reward=None), dict(noise=None), dict(y=None), dict(na=None), dict(ld=1019),
               dict(B=-1), dict(mw=-1), dict(N=0), dict(N=19), dict(agent=-1), dict(agent=20), dict(tau=0.0), dict(tau=-1.0),
               dict(tau=float("nan")), dict(tau=float("inf")), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(a=_mlp(size=8)),
               dict(c=_mlp(K=1060, O=1, size=8)), dict(a=_mlp(ptr=None)), dict(c=_mlp(K=1060, O=1, ptr=None)), dict(a=_mlp(K=50))):
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(a=_mlp(K=65), c=_mlp(K=19 * 67, O=1), N=19, ld=19 * 65), dict(a=_mlp(K=62), c=_mlp(K=21 * 64, O=1), N=21, ld=21 * 62),
               dict(a=_mlp(H1=257)), dict(a=_mlp(H2=257)), dict(c=_mlp(K=1060, H1=257, O=1)), dict(c=_mlp(K=1060, H2=257, O=1)),
               dict(a=_mlp(O=1)), dict(a=_mlp(O=3)), dict(c=_mlp(K=1060, O=2))):
        assert call(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert call(B=0) == nat.MDR_OK      # zero rows: nothing to launch


def test_gradient_calls_refuse_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    actor, critic = _mlp(), _mlp(K=20 * 53, O=1)

    def ccall(c=critic, state=p, ld=1020, action=p, B=16, N=20, y=p, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_maddpg_critic_grad(C.byref(c) if c is not None else None, state, ld, action, None, B, N, y, mw, ws, grad, loss, None, None)

    for kw in (dict(c=None), dict(state=None), dict(action=None), dict(y=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ld=1019),
               dict(B=-1), dict(mw=-1), dict(N=0), dict(N=19), dict(ws=C.c_void_p(0x1004)), dict(c=_mlp(K=1060, O=1, size=8)),
               dict(c=_mlp(K=1060, O=1, ptr=None)), dict(c=_mlp(K=40, O=1))):
        assert ccall(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(c=_mlp(K=1300, O=1), ld=1300), dict(c=_mlp(K=1060, H1=257, O=1)), dict(c=_mlp(K=1060, H2=257, O=1)), dict(c=_mlp(K=1060, O=2)),
               dict(c=_mlp(K=67, O=1), N=1, ld=65)):
        assert ccall(**kw) == nat.MDR_ERR_UNSUPPORTED, kw

    def acall(a=actor, c=critic, state=p, ld=1020, action=p, B=16, N=20, agent=19, noise=p, tau=1.0, pse=1e-3, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_maddpg_actor_grad(C.byref(a) if a is not None else None, C.byref(c) if c is not None else None, state, ld, action, None,
                                         B, N, agent, noise, C.c_float(tau), C.c_float(pse), mw, ws, grad, loss, None, None, None)

    for kw in (dict(a=None), dict(c=None), dict(state=None), dict(action=None), dict(noise=None), dict(ws=None), dict(grad=None),
               dict(loss=None), dict(ld=1019), dict(B=-1), dict(mw=-1), dict(N=0), dict(N=19), dict(agent=-1), dict(agent=20), dict(tau=0.0),
               dict(tau=float("nan")), dict(pse=float("nan")), dict(pse=float("inf")), dict(ws=C.c_void_p(0x1008)), dict(a=_mlp(size=8)),
               dict(a=_mlp(ptr=None)), dict(c=_mlp(K=1060, O=1, ptr=None)), dict(a=_mlp(K=50))):
        assert acall(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(a=_mlp(H1=257)), dict(a=_mlp(O=1)), dict(c=_mlp(K=1060, H2=257, O=1)), dict(c=_mlp(K=1060, O=2)),
               dict(a=_mlp(K=65), c=_mlp(K=19 * 67, O=1), N=19, ld=19 * 65, agent=0)):
        assert acall(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
