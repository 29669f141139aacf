"""The CPU side of the TarMAC-PPO update step: the yardstick of the gradient kernels (tests/tarmac_ppo_ref.py) held to its own
conditions, TarMACPPOLearner's torch backend against a literal transcription of agents/tarmac_ppo.py:152-207, from_config, the
host-only entry points, the ctypes mirror of mdr_tarmac_net_t and the argument checks that need no device."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from mdr_amd import _native as nat
from mdr_amd import tarmac_ppo as tp
from mdr_amd.tarmac import TarMACActor, TarMACCritic
from tests import tarmac_ppo_ref as pr
from tests import tarmac_ref as tr
from tests.test_abi import _header, _struct_fields

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tr.load_cases()


@pytest.mark.parametrize("name", pr.ONE_HOP)
def test_recorded_cases_meet_the_conditions(name):
    """``build`` asserts the ReLU condition, the ratios and the branches; here: the float32 CPU evaluation - the yardstick - is itself
    within a few 1e-6 of float64, and the reached tensors are those of parameters() less msg_state2state."""
    d = pr.recorded(name)
    assert d["margin"] > pr.RELU_MARGIN
    assert max(d["yard"].values()) < 1e-5
    reached = [n for n, _ in d["actor"].named_parameters() if "msg_state2state" not in n]
    assert sorted(d["grad"]) == sorted(reached)
    assert np.isfinite(d["loss"]) and all(np.isfinite(g).all() for g in d["grad"].values())


@pytest.mark.parametrize("name", sorted(pr.SYNTHETIC))
def test_synthetic_seeds_are_the_first_that_meet_the_relu_condition(name):
    weights, N, B, _, seed = pr.SYNTHETIC[name]
    assert pr.first_seed(weights, N, B) == seed
    assert pr.synthetic(name)["margin"] > pr.RELU_MARGIN


def test_defect_keys_meet_the_relu_condition_and_silence_senders():
    for step in pr.DEFECT_STEPS:
        d = pr.recorded("f22_n20_c10", step)
        assert 10 <= int(d["dead"].sum()) <= 40          # 80 senders at 0.3
    assert not np.array_equal(pr.recorded("f22_n20_c10", pr.DEFECT_STEPS[0])["dead"], pr.recorded("f22_n20_c10", pr.DEFECT_STEPS[1])["dead"])


def _small_batch(T=6, E=4, N=5, F=9, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"state": torch.randn((T + 1, E * N, F), generator=g), "action": torch.randint(0, 2, (T, E * N), generator=g),
            "a_prob": 0.3 + 0.4 * torch.rand((T, E * N), generator=g), "return": torch.randn((T, E * N), generator=g)}


def _transcription(actor, critic, batch, N, lr_actor, lr_critic, clip_param, max_grad_norm, ppo_update_time, indices):
    """agents/tarmac_ppo.py:152-207, line for line, on [time step, agent, ...] tensors; ``indices`` replaces the BatchSampler."""
    T = batch["state"].shape[0] - 1
    state = batch["state"][:T].reshape(-1, N, batch["state"].shape[-1])
    action = batch["action"].reshape(-1, N, 1)
    old_action_log_prob = batch["a_prob"].reshape(-1, N, 1)
    Gt = batch["return"].reshape(-1, N, 1)
    actor_optimizer = torch.optim.Adam(actor.parameters(), lr_actor)
    critic_net_optimizer = torch.optim.Adam(critic.parameters(), lr_critic)
    action_losses, value_losses = [], []
    for i in range(ppo_update_time):
        for index in indices[i]:
            Gt_index = Gt[index]
            V = critic(state[index]).unsqueeze(2)
            delta = Gt_index - V
            advantage = delta.detach()
            action_prob = actor(state[index])
            action_prob = action_prob.gather(2, action[index])
            ratio = action_prob / old_action_log_prob[index]
            clipped_ratio = torch.clamp(ratio, 1 - clip_param, 1 + clip_param)
            surr1 = ratio * advantage
            surr2 = clipped_ratio * advantage
            action_loss = -torch.min(surr1, surr2).mean()
            actor_optimizer.zero_grad()
            action_losses.append(action_loss.detach())
            action_loss.backward()
            nn.utils.clip_grad_norm_(actor.parameters(), max_grad_norm)
            actor_optimizer.step()
            value_loss = torch.pow(delta, 2).mean(0).mean(0)
            critic_net_optimizer.zero_grad()
            value_losses.append(value_loss.detach())
            value_loss.backward()
            nn.utils.clip_grad_norm_(critic.parameters(), max_grad_norm)
            critic_net_optimizer.step()
    return torch.stack(action_losses).mean(), torch.stack(value_losses).mean()


def test_torch_backend_is_the_reference_update_bit_for_bit():
    T, E, N, F = 6, 4, 5, 9
    batch = _small_batch(T, E, N, F)
    torch.manual_seed(11)
    actor = TarMACActor(F, num_key=4, num_value=8, hidden_state_size=12, number_agents_comm=3, attention="dense")
    critic = TarMACCritic(N, F, 16)
    actor_ref, critic_ref = copy.deepcopy(actor), copy.deepcopy(critic)
    learner = tp.TarMACPPOLearner(actor, critic, 1e-3, 2e-3, clip_param=0.2, max_grad_norm=0.5, ppo_update_time=2, batch_size=10, backend="torch")
    assert not learner.uses_kernels(10)
    indices = [learner.minibatches(T * E, 7, epoch) for epoch in range(2)]
    assert [len(i) for i in indices[0]] == [10, 10, 4]
    a_loss, c_loss, count = learner.update(batch, seed=7)
    a_ref, c_ref = _transcription(actor_ref, critic_ref, batch, N, 1e-3, 2e-3, 0.2, 0.5, 2, indices)
    assert count == 6 and learner.training_step == 6
    for (n, p), q in zip(list(actor.named_parameters()) + list(critic.named_parameters()),
                         list(actor_ref.parameters()) + list(critic_ref.parameters())):
        assert torch.equal(p, q), n
    assert actor.comm.msg_state2state[0].weight.grad is None
    np.testing.assert_allclose(float(a_loss), float(a_ref), rtol=1e-6)
    np.testing.assert_allclose(float(c_loss), float(c_ref), rtol=1e-6)


def test_from_config_reads_the_reference_keys():
    with open(os.path.join(GOLDEN, "tarmac_ppo_prop.json")) as f:
        prop = json.load(f)["TarMAC_PPO_prop"]
    actor = TarMACActor.from_config(prop, 51, attention="dense")
    critic = TarMACCritic(20, 51, prop["critic_hidden_layer_size"])
    learner = tp.TarMACPPOLearner.from_config(prop, actor, critic, backend="torch")
    assert (learner.clip_param, learner.max_grad_norm, learner.ppo_update_time, learner.batch_size) == (0.2, 0.5, 10, 256)
    assert learner.actor_optimizer.defaults["lr"] == 1e-3 and learner.critic_optimizer.defaults["lr"] == 1e-3
    with pytest.raises(ValueError):
        tp.TarMACPPOLearner.from_config(prop, actor, critic, backend="cuda")
    with pytest.raises(ValueError):                                   # the kernels run on the GPU: a CPU actor is refused by name
        tp.TarMACPPOLearner.from_config(prop, actor, critic, backend="hip")
    import mdr_amd
    assert mdr_amd.TarMACPPOLearner is tp.TarMACPPOLearner and mdr_amd.tarmac_ppo is tp


def test_ctypes_mirror_of_mdr_tarmac_net_matches_header():
    assert _struct_fields(_header(), "mdr_tarmac_net") == [f[0] for f in nat.MdrTarmacNet._fields_]


def _net(F, H, K, V, with_comm=1, hops=1, mode=0, size=None):
    return nat.MdrTarmacNet(C.sizeof(nat.MdrTarmacNet) if size is None else size, F, H, K, V, 10, mode, hops, with_comm, 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_grad_floats_is_the_sum_over_the_reached_parameters(name):
    lib = nat.load()
    case = CASES[name]
    net = _net(case["F"], case["H"], case["K"], case["V"], int(case["with_comm"]), case["hops"], case["mode"])
    if case["hops"] != 1:
        assert lib.mdr_tarmac_net_grad_floats(C.byref(net)) == -1
        return
    actor = tr.make_actor(case)
    reached = sum(p.numel() for n, p in actor.named_parameters() if "msg_state2state" not in n)
    assert lib.mdr_tarmac_net_grad_floats(C.byref(net)) == reached
    assert sum(p.numel() for p in tp._params(actor)) == reached
    # the flat order is the order of parameters()
    assert [id(p) for p in tp._params(actor)] == [id(p) for n, p in actor.named_parameters() if "msg_state2state" not in n]


def test_size_helpers_refuse_shapes_outside_the_limits():
    lib = nat.load()
    good = _net(51, 64, 8, 16)
    G = lib.mdr_tarmac_net_grad_floats(C.byref(good))
    assert G == 64 * 51 + 64 + 64 * 64 + 64 + 64 * 80 + 64 + 128 + 2 + 3 * (64 * 64 + 64) + 2 * (8 * 64 + 8) + 16 * 64 + 16
    for bad in ((65, 64, 8, 16), (51, 68, 8, 16), (51, 62, 8, 16), (51, 64, 20, 16), (51, 64, 6, 16), (51, 64, 8, 36), (51, 64, 8, 18),
                (0, 64, 8, 16), (51, 0, 8, 16), (51, 64, 0, 16)):
        assert lib.mdr_tarmac_net_grad_floats(C.byref(_net(*bad))) == -1, bad
        assert lib.mdr_tarmac_ppo_workspace_bytes(C.byref(_net(*bad)), 4, 20, 0) == -1, bad
    assert lib.mdr_tarmac_net_grad_floats(C.byref(_net(51, 64, 8, 16, hops=2))) == -1
    assert lib.mdr_tarmac_net_grad_floats(C.byref(_net(51, 64, 8, 16, mode=2))) == -1
    assert lib.mdr_tarmac_net_grad_floats(C.byref(_net(51, 64, 8, 16, size=8))) == -1
    assert lib.mdr_tarmac_net_grad_floats(None) == -1
    # without communication K and V do not matter
    assert lib.mdr_tarmac_net_grad_floats(C.byref(_net(22, 64, 0, 0, with_comm=0))) == 64 * 22 + 64 + 2 * (64 * 64 + 64) + 128 + 2
    stride = (G + 1 + 3) // 4 * 4 * 4

    def ws(rows, houses, wg):
        return lib.mdr_tarmac_ppo_workspace_bytes(C.byref(good), rows, houses, wg)

    def rest(agents):      # [x | comm], its gradient, q | k | v, its gradient, one float4 of statistics per agent
        return agents * (2 * 80 + 2 * 32 + 4) * 4

    assert ws(4, 20, 0) == 2 * 3 * stride + rest(80)              # 5 tiles, 3 pairs
    assert ws(4, 20, 2) == 2 * 2 * stride + rest(80)
    assert ws(0, 20, 0) == 2 * stride
    assert ws(10 ** 6, 20, 0) == 2 * 512 * stride + rest(20 * 10 ** 6)
    assert ws(-1, 20, 0) == -1 and ws(4, 0, 0) == -1 and ws(4, 20, -1) == -1 and ws(2 ** 31, 20, 0) == -1


def test_actor_loss_backward_checks_its_arguments_before_any_device_call():
    case = CASES["f22_n20_c10"]
    actor = tr.make_actor(case)
    state = torch.zeros((4, 20, 22))
    action, old, adv = torch.zeros((4, 20), dtype=torch.int64), torch.ones((4, 20)), torch.ones((4, 20))
    with pytest.raises(ValueError, match="on the GPU"):
        tp.actor_loss_backward(actor, state, action, old, adv)
    with pytest.raises(ValueError, match=r"\[M, N, F\]"):
        tp.actor_loss_backward(actor, state.view(80, 22), action, old, adv)
    with pytest.raises(ValueError, match="one hop"):
        tp.actor_loss_backward(tr.make_actor(CASES["f51_n50_c10_hops2"]), state, action, old, adv)
    assert not tp.supported(actor) and not tp.supported(nn.Linear(2, 2))
    assert "one hop" in tp._refusal(tr.make_actor(CASES["f51_n50_c10_hops2"]))
    wide = TarMACActor(22, hidden_state_size=68, attention="dense")
    assert "hidden_state_size" in tp._refusal(wide)
    assert "num_key" in tp._refusal(TarMACActor(22, num_key=20, attention="dense"))
