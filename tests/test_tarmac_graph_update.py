"""The constructor rules of ``TarMACPPOLearner`` / ``TarMACA2CLearner`` for ``sampler=`` and ``graph=`` (CPU; the graphs themselves:
tests/test_gpu_tarmac_graph_update.py).  ``graph=True`` is refused at construction, before anything could be captured: by the
backend, the sampler, the optimiser, a torch-autograd critic, and an actor the gradient kernels do not take."""
import inspect

import pytest
import torch

from mdr_amd import tarmac_a2c, tarmac_ppo
from mdr_amd.tarmac import TarMACActor, TarMACCritic

N, F = 5, 22
PPO_PROP = dict(lr_actor=1e-3, lr_critic=3e-3, clip_param=0.2, max_grad_norm=0.5, ppo_update_time=3, batch_size=16)
A2C_PROP = dict(tarmac_lr=7e-4, value_loss_coef=0.5, entropy_coef=0.01, tarmac_max_grad_norm=0.5, nb_tarmac_updates=3, tarmac_batch_size=16)


def _actor(**kw):
    return TarMACActor(F, hidden_state_size=16, number_agents_comm=2, **kw)


def _ppo(actor=None, **kw):
    return tarmac_ppo.TarMACPPOLearner(actor or _actor(), TarMACCritic(N, F), 1e-3, 3e-3, ppo_update_time=3, batch_size=16, **kw)


def _a2c(**kw):
    return tarmac_a2c.TarMACA2CLearner(tarmac_a2c.TarMACA2CPolicy(F), nb_updates=3, batch_size=16, **kw)


@pytest.mark.parametrize("make", [_ppo, _a2c])
def test_defaults_and_samplers(make):
    learner = make()
    assert learner.sampler == "torch" and learner.graph is False and learner.graph_captures == 0 and learner.graph_max_minibatches == 1024
    assert make(sampler="torch").sampler == "torch"
    philox = make(sampler="philox", graph_max_minibatches=7)
    assert philox.sampler == "philox" and philox.graph is False and philox.graph_max_minibatches == 7
    with pytest.raises(ValueError, match="sampler"):
        make(sampler="numpy")
    # torch's sampler cuts 48 env-steps as it always did: three minibatches of 16 that together hold every env-step once
    parts = learner.minibatches(48, 3, 0)
    assert [int(p.numel()) for p in parts] == [16, 16, 16]
    assert torch.equal(torch.sort(torch.cat(parts)).values, torch.arange(48))
    assert torch.equal(torch.cat(parts), torch.cat(make(sampler="torch").minibatches(48, 3, 0)))


def test_the_new_arguments_come_last_with_their_defaults():
    for fn in (tarmac_ppo.TarMACPPOLearner.__init__, tarmac_ppo.TarMACPPOLearner.from_config, tarmac_a2c.TarMACA2CLearner.__init__,
               tarmac_a2c.TarMACA2CLearner.from_config):
        params = inspect.signature(fn).parameters
        assert list(params)[-3:] == ["sampler", "graph", "graph_max_minibatches"]
        assert (params["sampler"].default, params["graph"].default, params["graph_max_minibatches"].default) == (None, False, 1024)


def test_from_config_hands_them_on():
    ppo = tarmac_ppo.TarMACPPOLearner.from_config(PPO_PROP, _actor(), TarMACCritic(N, F), sampler="philox", graph_max_minibatches=9)
    assert (ppo.sampler, ppo.graph, ppo.graph_max_minibatches, ppo.batch_size) == ("philox", False, 9, 16)
    a2c = tarmac_a2c.TarMACA2CLearner.from_config(A2C_PROP, tarmac_a2c.TarMACA2CPolicy(F), sampler="philox", graph_max_minibatches=9)
    assert (a2c.sampler, a2c.graph, a2c.graph_max_minibatches, a2c.batch_size) == ("philox", False, 9, 16)
    with pytest.raises(ValueError, match="graph=True"):
        tarmac_ppo.TarMACPPOLearner.from_config(PPO_PROP, _actor(), TarMACCritic(N, F), backend="torch", graph=True)
    with pytest.raises(ValueError, match="graph=True"):
        tarmac_a2c.TarMACA2CLearner.from_config(A2C_PROP, tarmac_a2c.TarMACA2CPolicy(F), backend="torch", graph=True)


@pytest.mark.parametrize("make", [_ppo, _a2c])
def test_graph_is_refused_by_backend_sampler_and_optimiser(make):
    with pytest.raises(ValueError, match=r"graph=True.*backend='torch'"):
        make(backend="torch", graph=True)
    with pytest.raises(ValueError, match=r"graph=True.*sampler='philox'"):
        make(sampler="torch", graph=True)
    with pytest.raises(ValueError, match="graph=True"):      # (the reason names FusedAdam where the networks are on a GPU)
        make(optimizer=torch.optim.Adam, graph=True)


def test_tarmac_ppo_graph_is_refused_by_critic_and_actor():
    with pytest.raises(ValueError, match=r"graph=True.*critic_backend='torch'.*autograd"):
        _ppo(critic_backend="torch", graph=True)
    with pytest.raises(ValueError, match=r"graph=True.*num_hops = 2"):
        _ppo(actor=_actor(num_hops=2), graph=True)
    with pytest.raises(ValueError, match=r"graph=True.*comm modes"):
        _ppo(actor=_actor(comm_mode="all", attention="gather"), graph=True)
    # the same actors without graph=True are what they were: the torch path takes them
    assert _ppo(actor=_actor(num_hops=2)).graph is False and _ppo(actor=_actor(comm_mode="all", attention="gather")).graph is False
