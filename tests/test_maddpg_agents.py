"""MADDPG with per-agent networks without a GPU: the fp64 restatement of the target with per-agent picks (tests/maddpg_agents_ref.py)
judged against maddpg_grad_ref's, what the learner and the C entry points refuse, and the checkpoint dict of ``saveDDPGDict``."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
from tests import maddpg_agents_ref as A
from tests import maddpg_grad_ref as R

N, F, H = 3, 5, 8
KEYS = {"actor_state_dict", "actor_optimizer_state_dict", "critic_state_dict", "critic_optimizer_state_dict", "tgt_actor_net_state_dict",
        "tgt_critic_net_state_dict", "lr_actor", "lr_critic", "gamma", "soft_tau"}


def _nets(n=N, f=F, h=H, seed=0):
    torch.manual_seed(seed)
    return [DDPGNetworkMLP(f, 2, h) for _ in range(n)], [DDPGNetworkMLP(n * (f + 2), 1, h) for _ in range(n)]


def _learner(actors, critics, **kw):
    kw.setdefault("backend", "torch")
    return MADDPGLearner(actors, critics, len(actors), 1e-3, 2e-3, batch_size=4, buffer_capacity=16, shared=False, **kw)


def _fill(learner, seed=1):
    g = torch.Generator().manual_seed(seed)
    n, f = learner.nb_agents, learner.num_state
    learner.buffer.push(torch.randn(8, n, f, generator=g), torch.randint(0, 2, (8, n), generator=g), torch.randn(8, n, generator=g),
                        torch.randn(8, n, f, generator=g))


@pytest.mark.parametrize("tau", A.TAUS)
@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_the_restatement_on_equal_and_on_distinct_nets(net, tau):
    n = net[0]
    agent = n - 1
    d, nets, first = A.draw(*net, rows=R.PARENT_ROWS, equal=True)
    assert first == 0
    shared = R.evaluate(R.inputs(R.PARENT_ROWS, *net), agent, tau)
    same = A.evaluate(d, nets, agent, tau)
    for k in ("y", "next_q", "next_action"):
        assert np.array_equal(same[k], shared[k]), k
    d, nets, first = A.draw(*net, rows=R.PARENT_ROWS)
    assert first == 0, "picks inside twice the bound on the first pass"
    if n > 1:
        own = A.evaluate(d, nets, agent, tau)
        assert not np.array_equal(own["next_action"], shared["next_action"])
        swapped = A.picks(d, (nets[0],) * n, tau)[:, 1]
        differ = int((swapped != own["next_action"][:, 1]).sum())
        print("MADDPG_AGENTS %s tau=%.1f net 0 and net 1 disagree on %d of agent 1's %d rows" % (net, tau, differ, R.PARENT_ROWS))
        assert 6 <= differ <= 39      # a kernel that used the wrong agent's net fails
        bnd = A.bound(d, nets, agent, tau)
        f32 = A.evaluate(d, nets, agent, tau, dtype=np.float32)
        assert np.array_equal(f32["next_action"], own["next_action"])
        assert R.worst(f32["y"], own["y"], bnd["y"]) <= 1.0 and R.worst(f32["next_q"], own["next_q"], bnd["next_q"]) <= 1.0


def test_learner_construction_is_refused():
    actors, critics = _nets()
    with pytest.raises(ValueError, match="sequences of nb_agents"):
        MADDPGLearner(actors[:2], critics, N, 1e-3, 1e-3, shared=False, backend="torch")
    with pytest.raises(ValueError, match="sequences of nb_agents"):
        MADDPGLearner(actors[0], critics[0], N, 1e-3, 1e-3, shared=False, backend="torch")
    with pytest.raises(ValueError, match="another shape"):
        MADDPGLearner(actors[:2] + [DDPGNetworkMLP(F, 2, H + 1)], critics, N, 1e-3, 1e-3, shared=False, backend="torch")
    with pytest.raises(ValueError, match="another shape"):
        MADDPGLearner(actors, critics[:2] + [DDPGNetworkMLP(N * (F + 2), 1, H + 1)], N, 1e-3, 1e-3, shared=False, backend="torch")
    many_a, many_c = _nets(33, 1, 2)
    with pytest.raises(ValueError, match="at most 32"):
        MADDPGLearner(many_a, many_c, 33, 1e-3, 1e-3, shared=False, backend="hip")
    assert MADDPGLearner(many_a, many_c, 33, 1e-3, 1e-3, shared=False, backend="torch").nb_agents == 33      # torch has no such limit
    with pytest.raises(ValueError, match="GPU"):
        MADDPGLearner(actors, critics, N, 1e-3, 1e-3, shared=False, backend="hip")      # CPU modules
    auto = _learner(actors, critics, backend="auto")
    assert not auto.uses_kernels(64) and not auto.shared and auto.actor is None
    assert [len(x) for x in (auto.actors, auto.critics, auto.tgt_actors, auto.tgt_critics, auto.actor_optimizers, auto.critic_optimizers)] == [N] * 6
    assert len({id(o) for o in auto.actor_optimizers}) == N and len({id(m) for m in auto.tgt_actors}) == N
    one = MADDPGLearner(actors[0], critics[0], N, 1e-3, 1e-3, backend="torch")
    assert one.shared and all(m is one.actor for m in one.actors) and all(m is one.tgt_critic for m in one.tgt_critics)
    assert all(o is one.critic_optimizer for o in one.critic_optimizers) and len(one.actors) == N
    cfg = dict(lr_actor=1e-3, lr_critic=1e-3, gamma=0.9, soft_tau=0.1, gumbel_softmax_tau=1.0, batch_size=4, buffer_capacity=16)
    assert MADDPGLearner.from_config(dict(cfg, DDPG_shared=False), actors, critics, N, backend="torch").shared is False
    assert MADDPGLearner.from_config(cfg, actors[0], critics[0], N, backend="torch").shared is True


def test_the_unshared_update_trains_every_agent_on_its_own_nets():
    actors, critics = _nets()
    for k in range(1, N):      # equal nets before the update
        actors[k].load_state_dict(actors[0].state_dict())
        critics[k].load_state_dict(critics[0].state_dict())
    learner = _learner(actors, critics)
    _fill(learner)
    before = [p.detach().clone() for p in learner.tgt_actors[0].parameters()]
    seen = []
    learner.before_step = lambda l, which, a: seen.append((which, a, [p.detach().clone() for t in l.tgt_actors for p in t.parameters()]))
    a_loss, c_loss = learner.update(seed=3)
    assert a_loss.shape == (N,) and c_loss.shape == (N,) and [(w, a) for w, a, _ in seen] == [(w, a) for a in range(N) for w in ("critic", "actor")]
    for _, _, snap in seen:      # the targets move only after the loop
        assert all(torch.equal(x, y) for x, y in zip(snap, seen[0][2]))
    assert all(torch.equal(x, y) for x, y in zip(seen[0][2][:6], before))
    for nets in (learner.actors, learner.critics):
        assert not torch.equal(nets[0].fc[0].weight, nets[1].fc[0].weight)      # each trained on its own minibatch
    for tgt, net, was in ((learner.tgt_actors[0], learner.actors[0], before),):
        for t, p, w in zip(tgt.parameters(), net.parameters(), was):
            torch.testing.assert_close(t, learner.soft_tau * p + (1 - learner.soft_tau) * w, rtol=0, atol=3 * 2.0 ** -24 * float(w.abs().max() + p.abs().max()))


def test_network_dict_round_trips_and_a_reference_dict_loads():
    learner = _learner(*_nets())
    _fill(learner)
    learner.update(seed=3)
    d = learner.network_dict()
    assert sorted(d) == list(range(N)) and all(set(e) == KEYS for e in d.values())
    assert list(d[1]["actor_state_dict"]) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"]
    fresh = _learner(*_nets(seed=9))
    fresh.load_network_dict(d)
    _fill(fresh)
    for i in range(N):
        for a, b in ((learner.actors, fresh.actors), (learner.critics, fresh.critics), (learner.tgt_actors, fresh.tgt_actors),
                     (learner.tgt_critics, fresh.tgt_critics)):
            assert all(torch.equal(x, y) for x, y in zip(a[i].parameters(), b[i].parameters()))
    fresh.training_step = learner.training_step
    for x, y in zip(learner.update(seed=4), fresh.update(seed=4)):      # Adam's moments came along
        assert torch.equal(x, y)
    # a dict in saveDDPGDict's shape, built by hand from plain modules and torch's own optimisers
    actors, critics = _nets(seed=5)
    hand = {i: {"actor_state_dict": actors[i].state_dict(), "actor_optimizer_state_dict": torch.optim.Adam(actors[i].parameters(), 1e-3).state_dict(),
                "critic_state_dict": critics[i].state_dict(),
                "critic_optimizer_state_dict": torch.optim.Adam(critics[i].parameters(), 2e-3).state_dict(),
                "tgt_actor_net_state_dict": actors[(i + 1) % N].state_dict(), "tgt_critic_net_state_dict": critics[(i + 1) % N].state_dict(),
                "lr_actor": 1e-3, "lr_critic": 2e-3, "gamma": 0.99, "soft_tau": 0.01} for i in range(N)}
    fresh.load_network_dict(hand)
    assert torch.equal(fresh.actors[2].fc[1].weight, actors[2].fc[1].weight) and torch.equal(fresh.tgt_actors[2].fc[1].weight, actors[0].fc[1].weight)
    with pytest.raises(ValueError, match="one entry per agent"):
        fresh.load_network_dict({0: hand[0]})
    shared = MADDPGLearner(actors[0], critics[0], N, 1e-3, 2e-3, backend="torch")
    ds = shared.network_dict()
    assert sorted(ds) == list(range(N)) and ds[2]["actor_state_dict"]["net.0.weight"].data_ptr() == ds[0]["actor_state_dict"]["net.0.weight"].data_ptr()
    shared.load_network_dict(hand)
    assert torch.equal(shared.actor.fc[0].weight, actors[0].fc[0].weight)


def test_the_entry_points_refuse_on_the_host():
    lib = nat.load()
    assert nat.MDR_ABI_VERSION == 5 == lib.mdr_abi_version() and nat.MDR_MAX_AGENT_NETS == 32
    assert len(lib.mdr_mlp_actors_sample.argtypes) == 14 and len(lib.mdr_maddpg_target_agents.argtypes) == 18
    p = 0x1000      # never dereferenced: every call below returns before a launch

    def descs(n, K=51, H1=256, H2=256, O=2):
        return (nat.MdrMlp * n)(*[nat.MdrMlp(C.sizeof(nat.MdrMlp), K, H1, H2, O, *([p] * 6)) for _ in range(n)])

    def act(d, n, rows=12, ld=51, obs=p, action=p):
        return lib.mdr_mlp_actors_sample(d, n, obs, ld, rows, C.c_uint64(1), C.c_uint64(2), None, 0, 0, action, p, p, None)

    inv, uns = nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED
    assert act(None, 3) == inv and act(descs(3), 0) == inv and act(descs(3), 3, rows=-1) == inv and act(descs(3), 3, rows=13) == inv
    assert act(descs(3), 3, ld=50) == inv and act(descs(3), 3, obs=None) == inv and act(descs(3), 3, action=None) == inv
    assert act(descs(33), 33, rows=33) == uns and act(descs(3, K=129), 3, ld=129) == uns and act(descs(3, H1=257), 3) == uns
    assert act(descs(3, O=1), 3) == uns
    odd = descs(3)
    odd[1].hidden2 = 255
    assert act(odd, 3) == uns
    assert act(descs(3), 3, rows=0) == nat.MDR_OK and act(descs(32), 32, rows=0) == nat.MDR_OK

    critic = nat.MdrMlp(C.sizeof(nat.MdrMlp), 3 * 53, 256, 256, 1, *([p] * 6))

    def tgt(d, n, N=3, agent=0, B=16, tau=1.0):
        return lib.mdr_maddpg_target_agents(d, n, C.byref(critic), p, 3 * 51, p, None, B, N, agent, p, C.c_float(tau), C.c_float(0.99), 0, p, p, p, None)

    assert tgt(None, 3) == inv and tgt(descs(2), 2) == inv and tgt(descs(3), 3, agent=3) == inv and tgt(descs(3), 3, B=-1) == inv
    assert tgt(descs(3), 3, tau=0.0) == inv and tgt(odd, 3) == uns and tgt(descs(33), 33, N=33) == uns
    assert tgt(descs(3), 3, B=0) == nat.MDR_OK
