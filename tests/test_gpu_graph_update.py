"""``graph=True`` of PPOLearner, MAPPOLearner and DQNLearner on the GPU: the update replayed from a captured graph gives the bits of
the eager ``sampler="philox"`` update - parameters, moments, step counts, losses -, captures once per batch shape, leaves no trace
when it captures, and refuses at construction or at the first update what it cannot replay."""
import pytest
import torch

from mdr_amd import dqn, mappo, ppo
from mdr_amd.optim import FusedAdam
from mdr_amd.rollout import ActorMLP, CriticMLP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, N = 51, 20


def _batch(T, A, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(state=torch.randn((T + 1, A, F), generator=g).to(DEV), action=torch.randint(0, 2, (T, A), generator=g).to(DEV),
                a_prob=(0.2 + 0.6 * torch.rand((T, A), generator=g)).to(DEV), **{"return": torch.randn((T, A), generator=g).to(DEV)})


def _nets(kind, seed=0, hidden=(100, 100)):
    torch.manual_seed(seed)
    actor = ActorMLP(F, layers=hidden).to(DEV)
    critic = CriticMLP(F + (N - 1 if kind == "mappo" else 0), layers=hidden).to(DEV)
    return actor, critic


def _ppo_learner(kind, sd, **kw):
    actor, critic = _nets(kind)
    actor.load_state_dict(sd[0])
    critic.load_state_dict(sd[1])
    cls = mappo.MAPPOLearner if kind == "mappo" else ppo.PPOLearner
    kw.setdefault("optimizer", FusedAdam)
    return cls(actor, critic, 1e-3, 3e-3, batch_size=64, ppo_update_time=3, **kw)


def _ppo_state(L):
    out = [p.detach().clone() for p in list(L.actor.parameters()) + list(L.critic.parameters())]
    for opt in (L.actor_optimizer, L.critic_optimizer):
        out += [opt._exp_avg.clone(), opt._exp_avg_sq.clone()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _steps(opt):
    return sorted({float(st["step"]) for st in opt.state.values() if st})


@pytest.mark.parametrize("kind", ["ppo", "mappo"])
def test_graphed_update_gives_the_eager_bits(kind):
    """n = 300 transitions in minibatches of 64 (four full ones and a tail of 44), three epochs; two updates on fresh batch tensors
    under different seeds through ONE capture, then a batch of another shape through a second."""
    a0, c0 = _nets(kind, seed=3)
    sd = (a0.state_dict(), c0.state_dict())
    eager, graphed = _ppo_learner(kind, sd, sampler="philox"), _ppo_learner(kind, sd, graph=True)
    assert graphed.sampler == "philox" and graphed.graph_captures == 0
    done = 0
    for call, (T, seed, captures) in enumerate(((5, 11, 1), (5, 12, 1), (4, 13, 2))):
        batch = _batch(T, 60, 100 + call)      # a fresh tensor at another address every call
        ea, ec, en = eager.update(batch, seed=seed)
        ga, gc, gn = graphed.update({k: v.clone() for k, v in batch.items()}, seed=seed)
        done += 3 * -(-T * 60 // 64)
        assert en == gn == 3 * -(-T * 60 // 64)
        assert torch.equal(ea, ga) and torch.equal(ec, gc) and bool(torch.isfinite(ga)) and bool(torch.isfinite(gc))
        assert _same(_ppo_state(eager), _ppo_state(graphed))
        assert eager.training_step == graphed.training_step == done
        for opt_e, opt_g in ((eager.actor_optimizer, graphed.actor_optimizer), (eager.critic_optimizer, graphed.critic_optimizer)):
            assert _steps(opt_e) == _steps(opt_g) == [float(done)] and opt_g._t == done
        assert graphed.graph_captures == captures
    assert done == 15 + 15 + 12


def test_philox_and_torch_samplers_cut_the_same_way():
    a0, c0 = _nets("ppo")
    sd = (a0.state_dict(), c0.state_dict())
    for sampler in ("torch", "philox"):
        L = _ppo_learner("ppo", sd, sampler=sampler)
        for epoch in range(2):
            parts = L.minibatches(300, 5, epoch)
            assert [int(p.numel()) for p in parts] == [64, 64, 64, 64, 44]
            assert all(p.dtype == torch.int64 and p.device.type == "cuda" for p in parts)
            assert torch.equal(torch.sort(torch.cat(parts)).values, torch.arange(300, device=DEV))
    assert not torch.equal(torch.cat(L.minibatches(300, 5, 0)), torch.cat(L.minibatches(300, 5, 1)))
    assert not torch.equal(torch.cat(L.minibatches(300, 5, 0)), torch.cat(L.minibatches(300, 6, 0)))


@pytest.mark.parametrize("kind", ["ppo", "mappo"])
def test_capture_leaves_no_trace(kind):
    a0, c0 = _nets(kind, seed=4)
    L = _ppo_learner(kind, (a0.state_dict(), c0.state_dict()), graph=True)
    L.update(_batch(2, 40, 1), seed=1)      # nonzero moments and counts (two minibatches x three epochs; one capture)
    before, t0 = _ppo_state(L), L.training_step
    steps = (_steps(L.actor_optimizer), _steps(L.critic_optimizer), L.actor_optimizer._t, L.critic_optimizer._t)
    L._capture((5, 60, F))      # runs the warm-up pass and the capture, replays nothing
    torch.cuda.synchronize()
    assert L.graph_captures == 2
    assert _same(before, _ppo_state(L)) and L.training_step == t0 == 6
    assert steps == (_steps(L.actor_optimizer), _steps(L.critic_optimizer), L.actor_optimizer._t, L.critic_optimizer._t) == ([6.0], [6.0], 6, 6)


def test_ppo_refusals_leave_the_parameters_alone():
    a0, c0 = _nets("ppo")
    sd = (a0.state_dict(), c0.state_dict())
    with pytest.raises(ValueError, match="FusedAdam"):
        _ppo_learner("ppo", sd, graph=True, optimizer=torch.optim.Adam)
    with pytest.raises(ValueError, match="torch"):
        _ppo_learner("ppo", sd, graph=True, backend="torch")
    with pytest.raises(ValueError, match="sampler"):
        _ppo_learner("ppo", sd, graph=True, sampler="torch")
    with pytest.raises(ValueError):
        _ppo_learner("ppo", sd, sampler="numpy")
    wide_a, wide_c = _nets("ppo", hidden=(129, 129))
    for backend in ("auto", "hip"):
        with pytest.raises(ValueError):
            ppo.PPOLearner(wide_a, wide_c, 1e-3, 3e-3, backend=backend, optimizer=FusedAdam, graph=True)
    batch = _batch(5, 60, 1)
    hooked = _ppo_learner("ppo", sd, graph=True)
    hooked.before_clip = lambda learner: None
    capped = _ppo_learner("ppo", sd, graph=True, graph_max_minibatches=4)      # 300 transitions are five minibatches
    for L in (hooked, capped):
        before = _ppo_state(L)
        with pytest.raises(ValueError, match="before_clip|graph_max_minibatches"):
            L.update(batch, seed=0)
        assert _same(before, _ppo_state(L)) and L.training_step == 0 and L.graph_captures == 0
    capped.graph_max_minibatches = 5
    assert capped.update(batch, seed=0)[2] == 15


# -- DQN / DDQN -------------------------------------------------------------------------------------------------------------------------
def _dqn_learner(double, sd, **kw):
    torch.manual_seed(0)
    net = dqn.QNetworkMLP(F).to(DEV)
    net.load_state_dict(sd)
    kw.setdefault("optimizer", FusedAdam)
    return dqn.DQNLearner(net, 1e-3, buffer_capacity=1024, batch_size=256, double=double, **kw)


def _dqn_state(L):
    out = [p.detach().clone() for p in list(L.policy_net.parameters()) + list(L.target_net.parameters())]
    return out + [L.optimizer._exp_avg.clone(), L.optimizer._exp_avg_sq.clone()]


def _transitions(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, F), generator=g).to(DEV), torch.randint(0, 2, (n,), generator=g).to(DEV), torch.randn(n, generator=g).to(DEV),
            torch.randn((n, F), generator=g).to(DEV))


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
def test_graphed_dqn_update_gives_the_eager_bits(double):
    torch.manual_seed(5)
    sd = dqn.QNetworkMLP(F).state_dict()
    eager, graphed = _dqn_learner(double, sd, sampler="philox"), _dqn_learner(double, sd, graph=True)
    rows = _transitions(200, 1)
    for L in (eager, graphed):
        L.buffer.push(*rows)
        assert L.update(seed=1) is None      # 200 < 256 transitions: no update, and no capture
    assert graphed.graph_captures == 0 and graphed.training_step == 0
    updates = 0
    for more, seeds in ((100, (7,)), (200, (8, 9))):      # 300 stored, one update; 500 stored, two
        rows = _transitions(more, 2 + more)
        for L in (eager, graphed):
            L.buffer.push(*rows)
        for seed in seeds:
            le, lg = eager.update(seed=seed), graphed.update(seed=seed)
            updates += 1
            assert torch.equal(le, lg) and bool(torch.isfinite(lg))
            assert _same(_dqn_state(eager), _dqn_state(graphed))
            assert eager.training_step == graphed.training_step == updates
            assert _steps(eager.optimizer) == _steps(graphed.optimizer) == [float(updates)] and graphed.optimizer._t == updates
    assert graphed.graph_captures == 1 and updates == 3
    assert not _same(_dqn_state(graphed)[6:12], [p.detach() for p in graphed.policy_net.parameters()])      # the target net lags the policy net


def test_dqn_capture_leaves_no_trace_and_refusals():
    torch.manual_seed(6)
    sd = dqn.QNetworkMLP(F).state_dict()
    L = _dqn_learner(True, sd, graph=True)
    L.buffer.push(*_transitions(300, 3))
    L.update(seed=2)
    before, steps = _dqn_state(L), (_steps(L.optimizer), L.optimizer._t, L.training_step)
    L._capture()
    torch.cuda.synchronize()
    assert L.graph_captures == 2 and _same(before, _dqn_state(L))
    assert steps == (_steps(L.optimizer), L.optimizer._t, L.training_step) == ([1.0], 1, 1)
    with pytest.raises(ValueError, match="FusedAdam"):
        _dqn_learner(False, sd, graph=True, optimizer=torch.optim.Adam)
    with pytest.raises(ValueError, match="torch"):
        _dqn_learner(False, sd, graph=True, backend="torch")
    with pytest.raises(ValueError):
        dqn.DQNLearner(dqn.QNetworkMLP(F, layers=(129, 129)).to(DEV), 1e-3, optimizer=FusedAdam, graph=True)
    hooked = _dqn_learner(False, sd, graph=True)
    hooked.buffer.push(*_transitions(300, 3))
    hooked.before_step = lambda learner: None
    before = _dqn_state(hooked)
    with pytest.raises(ValueError, match="before_step"):
        hooked.update(seed=0)
    assert _same(before, _dqn_state(hooked)) and hooked.graph_captures == 0 and hooked.training_step == 0
