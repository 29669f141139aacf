"""``MADDPGLearner(sampler="philox")`` and ``graph=True`` on the GPU, in the manner of tests/test_gpu_graph_update.py: the update replayed
from a captured graph gives the bits of the eager ``sampler="philox"`` update - losses, every net and target, moments, step counts -
with shared and with per-agent networks, captures once, leaves no trace when it captures, captures again for another batch size, and
refuses at construction or at the first update what it cannot replay."""
import pytest
import torch

from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner, train_maddpg
from mdr_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _learner(shared, N=3, F=12, hidden=48, B=16, capacity=128, seed=0, **kw):
    """Equal seeds give equal nets: two learners built alike start from the same bits."""
    torch.manual_seed(seed)
    n = 1 if shared else N
    actors = [DDPGNetworkMLP(F, 2, hidden).to(DEV) for _ in range(n)]
    critics = [DDPGNetworkMLP(N * (F + 2), 1, hidden).to(DEV) for _ in range(n)]
    kw.setdefault("optimizer", FusedAdam)
    kw.setdefault("backend", "hip")
    return MADDPGLearner(actors[0] if shared else actors, critics[0] if shared else critics, N, 1e-3, 3e-3, batch_size=B, buffer_capacity=capacity,
                         shared=shared, **kw)


def _steps_rows(n, N, F, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, N, F), generator=g).to(DEV), torch.randint(0, 2, (n, N), generator=g).to(DEV), torch.randn((n, N), generator=g).to(DEV),
            torch.randn((n, N, F), generator=g).to(DEV))


def _nets(L):
    n = 1 if L.shared else L.nb_agents
    return L.actors[:n] + L.critics[:n], L.tgt_actors[:n] + L.tgt_critics[:n], L.actor_optimizers[:n] + L.critic_optimizers[:n]


def _state(L):
    nets, tgts, opts = _nets(L)
    out = [p.detach().clone() for m in nets + tgts for p in m.parameters()]
    for opt in opts:
        out += [opt._exp_avg.clone(), opt._exp_avg_sq.clone()]
    return out


def _counts(L):
    return [(sorted({float(st["step"]) for st in opt.state.values() if st}), opt._t) for opt in _nets(L)[2]] + [L.training_step]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _targets_lag(L):
    nets, tgts, _ = _nets(L)
    return all(not torch.equal(p, t) for m, tm in zip(nets, tgts) for p, t in zip(m.fc[0].parameters(), tm.fc[0].parameters()))


def _compare(eager, graphed, seed):
    (ae, ce), (ag, cg) = eager.update(seed=seed), graphed.update(seed=seed)
    N = eager.nb_agents
    assert ag.shape == cg.shape == (N,) and torch.equal(ae, ag) and torch.equal(ce, cg)
    assert bool(torch.isfinite(ag).all()) and bool(torch.isfinite(cg).all())
    assert _same(_state(eager), _state(graphed))
    assert _counts(eager) == _counts(graphed)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "unshared"])
def test_graphed_update_gives_the_eager_bits(shared):
    N, F = 3, 12
    eager, graphed = _learner(shared, sampler="philox"), _learner(shared, graph=True)
    assert graphed.sampler == "philox" and _same(_state(eager), _state(graphed))
    rows = _steps_rows(10, N, F, 1)
    for L in (eager, graphed):
        L.buffer.push(*rows)
        assert L.update(seed=1) is None      # 10 < 16 env-steps: no update, and no capture
    assert graphed.graph_captures == 0 and graphed.training_step == 0
    initial = _state(graphed)
    updates = 0
    for more, seeds in ((30, (7,)), (60, (8, 9))):      # 40 stored: one update; 100 stored: two more
        rows = _steps_rows(more, N, F, 2 + more)
        for L in (eager, graphed):
            L.buffer.push(*rows)
        for seed in seeds:
            _compare(eager, graphed, seed)
            updates += 1
            per_net = N if shared else 1      # a shared net steps once per agent, an agent's own net once
            assert _counts(graphed)[:-1] == [([float(updates * per_net)], updates * per_net)] * len(_nets(graphed)[2])
            assert graphed.training_step == updates
    assert graphed.graph_captures == 1 and updates == 3
    assert not _same(initial, _state(graphed)) and _targets_lag(graphed)
    # the blend ran once per update: after one more update from equal nets the target is tau of the way, not 0 and not N tau
    one = _learner(shared, graph=True, seed=4)
    one.buffer.push(*_steps_rows(40, N, F, 9))
    before = [p.detach().clone() for p in one.tgt_critics[0].parameters()]
    one.update(seed=3)
    for t0, t1, p in zip(before, one.tgt_critics[0].parameters(), one.critics[0].parameters()):
        assert torch.allclose(t1, (1 - one.soft_tau) * t0 + one.soft_tau * p.detach(), rtol=1e-5, atol=1e-7)
    before = [p.detach().clone() for p in one.tgt_actors[0].parameters()]
    one.update(seed=4)
    for t0, t1, p in zip(before, one.tgt_actors[0].parameters(), one.actors[0].parameters()):
        assert torch.allclose(t1, (1 - one.soft_tau) * t0 + one.soft_tau * p.detach(), rtol=1e-5, atol=1e-7)


def test_graphed_update_at_the_references_shape():
    """N = 20, F = 51, hidden 256, B = 64: the workspace and the LDS sizes are the real ones."""
    kw = dict(N=20, F=51, hidden=256, B=64, capacity=128)
    eager, graphed = _learner(True, sampler="philox", **kw), _learner(True, graph=True, **kw)
    rows = _steps_rows(80, 20, 51, 5)
    for L in (eager, graphed):
        L.buffer.push(*rows)
    _compare(eager, graphed, 11)
    assert graphed.graph_captures == 1 and _targets_lag(graphed)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "unshared"])
def test_philox_sampler_trains_like_the_torch_sampler(shared):
    N, F, B = 3, 12, 16
    rows = _steps_rows(40, N, F, 6)
    draws = []
    for sampler in ("torch", "philox", None):
        L = _learner(shared, sampler=sampler)
        assert L.sampler == (sampler or "torch") and not L.graph
        L.buffer.push(*rows)
        before = _state(L)
        d = L.draws(3)
        draws.append(d)
        assert d[0].shape == (N, B) and d[0].dtype == torch.int64 and d[1].shape == (N, B, N, 2) and d[2].shape == (N, B, 2)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in d[1:])
        assert int(d[0].min()) >= 0 and int(d[0].max()) < 40 and all(len(set(row.tolist())) == B for row in d[0])
        a_loss, c_loss = L.update(seed=3)
        assert a_loss.shape == c_loss.shape == (N,) and bool(torch.isfinite(a_loss).all()) and bool(torch.isfinite(c_loss).all())
        n = 1 if shared else N
        assert all(not torch.equal(x, y) for x, y in zip(before[:12 * n], _state(L)[:12 * n]))      # every actor and critic tensor moved
    assert not torch.equal(draws[0][0], draws[1][0])      # other draws of the same laws
    assert all(torch.equal(x, y) for x, y in zip(draws[0], draws[2]))      # the default is today's sampler


def test_philox_sampler_on_the_torch_backend():
    L = _learner(True, sampler="philox", backend="torch", optimizer=torch.optim.Adam)
    L.buffer.push(*_steps_rows(40, 3, 12, 6))
    a_loss, c_loss = L.update(seed=3)
    assert bool(torch.isfinite(a_loss).all()) and bool(torch.isfinite(c_loss).all())


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "unshared"])
def test_capture_leaves_no_trace(shared):
    L = _learner(shared, graph=True)
    L.buffer.push(*_steps_rows(40, 3, 12, 7))
    L.update(seed=2)
    before, counts = _state(L), _counts(L)
    L._capture()
    torch.cuda.synchronize()
    assert L.graph_captures == 2 and _same(before, _state(L)) and counts == _counts(L) and L.training_step == 1


def test_refusals_leave_the_learner_untouched():
    with pytest.raises(ValueError, match="FusedAdam"):
        _learner(True, graph=True, optimizer=torch.optim.Adam)
    with pytest.raises(ValueError, match="torch"):
        _learner(True, graph=True, backend="torch")
    with pytest.raises(ValueError, match="philox"):
        _learner(True, graph=True, sampler="torch")
    with pytest.raises(ValueError, match="sampler"):
        _learner(True, sampler="numpy")
    with pytest.raises(ValueError):
        _learner(True, graph=True, hidden=257)
    with pytest.raises(ValueError, match="graph=True"):
        _learner(True, graph=True, hidden=257, backend="auto")
    with pytest.raises(ValueError, match="graph=True"):
        _learner(False, graph=True, backend="auto")      # "auto" resolves to torch for per-agent nets
    hooked = _learner(True, graph=True)
    hooked.buffer.push(*_steps_rows(40, 3, 12, 3))
    hooked.before_step = lambda learner, which, agent: None
    before, counts = _state(hooked), _counts(hooked)
    with pytest.raises(ValueError, match="before_step"):
        hooked.update(seed=0)
    assert _same(before, _state(hooked)) and counts == _counts(hooked) and hooked.graph_captures == 0 and hooked.training_step == 0


def test_another_batch_size_captures_again():
    N, F = 3, 12
    eager, graphed = _learner(True, sampler="philox"), _learner(True, graph=True)
    rows = _steps_rows(50, N, F, 8)
    for L in (eager, graphed):
        L.buffer.push(*rows)
    _compare(eager, graphed, 1)
    for L in (eager, graphed):
        L.batch_size = 24
    _compare(eager, graphed, 2)
    _compare(eager, graphed, 3)
    assert graphed.graph_captures == 2 and graphed._graph.index.shape == (N, 24)


def test_from_config_passes_sampler_and_graph_through():
    torch.manual_seed(0)
    prop = dict(lr_actor=1e-3, lr_critic=3e-3, gamma=0.99, soft_tau=0.01, gumbel_softmax_tau=1.0, batch_size=16, buffer_capacity=64)
    L = MADDPGLearner.from_config(prop, DDPGNetworkMLP(12, 2, 48).to(DEV), DDPGNetworkMLP(3 * 14, 1, 48).to(DEV), 3, backend="hip", optimizer=FusedAdam,
                                  graph=True)
    assert L.graph and L.sampler == "philox"
    L = MADDPGLearner.from_config(prop, DDPGNetworkMLP(12, 2, 48).to(DEV), DDPGNetworkMLP(3 * 14, 1, 48).to(DEV), 3, sampler="philox")
    assert not L.graph and L.sampler == "philox"


def test_train_maddpg_runs_a_graphed_learner():
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 3
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=2, device=DEV, seed=11)
    env.reset(episode=0)
    F = env.obs_vector_length()
    torch.manual_seed(2)
    actor, critic = DDPGNetworkMLP(F, 2, 48).to(DEV), DDPGNetworkMLP(3 * (F + 2), 1, 48).to(DEV)
    learner = MADDPGLearner(actor, critic, 3, 1e-3, 3e-3, batch_size=4, buffer_capacity=64, backend="hip", optimizer=FusedAdam, graph=True)
    a_losses, c_losses = train_maddpg(env, learner, nb_steps=6, update_every=2, random_steps=2)
    assert a_losses.shape == c_losses.shape == (3, 3)      # updates after steps 2, 4 and 6
    assert bool(torch.isfinite(a_losses).all()) and bool(torch.isfinite(c_losses).all())
    assert learner.graph_captures == 1 and learner.training_step == 3
