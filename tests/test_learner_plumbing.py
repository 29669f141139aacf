"""mdr_amd._learner on the CPU: what the learners share and no GPU test can hold to a host-side contract - the three ways a flat
gradient is published, clip + step, the replay ring under both of its subclasses, the minibatch cut."""
from collections import deque

import pytest
import torch
import torch.nn as nn

from mdr_amd import _learner as L
from mdr_amd.dqn import DeviceReplayBuffer
from mdr_amd.maddpg import JointReplayBuffer


def _params_and_flat():
    params = [nn.Parameter(torch.zeros(2, 3)), nn.Parameter(torch.zeros(3))]
    return params, torch.arange(1.0, 10.0)


def _views(params, flat):
    return [flat[:6].view(2, 3), flat[6:9]]


@pytest.mark.parametrize("mode", [L.KEEP, L.REPLACE, L.REBIND])
def test_publish_where_grad_is_none(mode):
    params, flat = _params_and_flat()
    L.publish(params, flat, mode)
    for p, view in zip(params, _views(params, flat)):
        assert p.grad.data_ptr() == view.data_ptr() and p.grad.shape == p.shape and torch.equal(p.grad, view)
    flat += 1.0      # a view, not a copy
    assert torch.equal(params[1].grad, flat[6:9])


@pytest.mark.parametrize("mode", [L.KEEP, L.REPLACE, L.REBIND])
def test_publish_where_grad_is_already_the_view(mode):
    params, flat = _params_and_flat()
    L.publish(params, flat, mode)
    before = [p.grad for p in params]
    version = flat._version
    L.publish(params, flat, mode)
    assert flat._version == version      # nothing was copied onto the buffer
    for p, was, view in zip(params, before, _views(params, flat)):
        assert p.grad.data_ptr() == view.data_ptr() and torch.equal(p.grad, view)
        # KEEP and REBIND leave the object alone; REPLACE assigns a fresh view of the same memory, as tarmac_a2c always did
        assert (p.grad is was) == (mode != L.REPLACE)


@pytest.mark.parametrize("mode,stays,receives", [(L.KEEP, True, True), (L.REPLACE, False, True), (L.REBIND, False, False)])
def test_publish_where_grad_is_a_foreign_tensor(mode, stays, receives):
    params, flat = _params_and_flat()
    foreign = [torch.full_like(p, -1.0) for p in params]
    for p, g in zip(params, foreign):
        p.grad = g
    L.publish(params, flat, mode)
    for p, g, view in zip(params, foreign, _views(params, flat)):
        assert (p.grad is g) == stays
        assert stays or p.grad.data_ptr() == view.data_ptr()
        assert torch.equal(g, view if receives else torch.full_like(g, -1.0))
        assert torch.equal(p.grad, view)      # whichever tensor it is, it holds the gradient


def test_flat_grad_is_kept_with_the_module_and_reallocated_on_another_size():
    net = nn.Linear(2, 2)
    flat = L.flat_grad(net, 6, torch.device("cpu"))
    assert flat.shape == (6,) and flat.dtype == torch.float32 and net._mdr_flat_grad is flat
    assert L.flat_grad(net, 6, torch.device("cpu")) is flat
    assert L.flat_grad(net, 8, torch.device("cpu")) is not flat and net._mdr_flat_grad.numel() == 8


def _toy(seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [nn.Parameter(torch.randn(shape, generator=g)) for shape in ((4, 3), (4,), (2, 4))]
    for p in params:
        p.grad = 3.0 * torch.randn(p.shape, generator=g)      # a norm well above the clip
    return params


def test_clip_and_step_is_clip_grad_norm_then_step():
    mine, theirs = _toy(), _toy()
    opt_mine, opt_theirs = torch.optim.Adam(mine, 1e-2), torch.optim.Adam(theirs, 1e-2)
    for _ in range(2):
        L.clip_and_step(opt_mine, mine, 0.5, target=[torch.zeros(1)], tau=0.1)      # the fused keywords are not torch.optim.Adam's: ignored
        nn.utils.clip_grad_norm_(theirs, 0.5)
        opt_theirs.step()
    for a, b in zip(mine, theirs):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
    assert float(torch.sqrt(sum((p.grad ** 2).sum() for p in mine))) <= 0.5 * (1 + 1e-5)      # and the clip did bite


def test_clip_and_step_of_its_two_halves():
    mine, theirs = _toy(1), _toy(1)
    opt_mine, opt_theirs = torch.optim.Adam(mine, 1e-2), torch.optim.Adam(theirs, 1e-2)
    L.clip(opt_mine, mine, 0.5)
    L.step(opt_mine, 0.5)
    L.clip_and_step(opt_theirs, theirs, 0.5)
    assert all(torch.equal(a, b) for a, b in zip(mine, theirs))


def test_blend():
    target, new = [torch.ones(3), torch.zeros(2)], [torch.full((3,), 3.0), torch.ones(2)]
    L.blend(target, new, 0.25)
    assert torch.equal(target[0], torch.full((3,), 1.5)) and torch.equal(target[1], torch.full((2,), 0.25))


def _ring(kind):
    if kind == "dqn":
        return DeviceReplayBuffer(5, 2, "cpu"), ()
    return JointReplayBuffer(5, 3, 2, "cpu"), (3,)


def _rows(first, n, row):
    """Entries first .. first + n - 1, every element of entry k holding k (next_state: k + 0.5, action: k, reward: -k)."""
    k = torch.arange(first, first + n, dtype=torch.float32)
    state = k.reshape((n,) + (1,) * (len(row) + 1)).expand((n,) + row + (2,)).contiguous()
    flat = k.reshape((n,) + (1,) * len(row)).expand((n,) + row).contiguous()
    return state, flat.to(torch.int64), -flat, state + 0.5


@pytest.mark.parametrize("kind", ["dqn", "maddpg"])
def test_ring_against_a_deque(kind):
    buf, row = _ring(kind)
    want = deque(maxlen=5)
    assert len(buf) == 0 and buf.chronological().numel() == 0
    first = 0
    for n, pos in ((3, 3), (4, 2), (7, 2)):      # a push that fits, one that wraps, one larger than the capacity: its last 5 stay
        state, action, reward, next_state = _rows(first, n, row)
        buf.push(state, action, reward, next_state)
        want.extend(range(first, first + n))
        first += n
        assert len(buf) == len(want) and buf._pos == pos
        order = buf.chronological()
        assert order.dtype == torch.int64 and sorted(order.tolist()) == list(range(len(want)))
        k = torch.tensor(list(want), dtype=torch.float32)
        assert torch.equal(buf.state[order], k.reshape((-1,) + (1,) * (len(row) + 1)).expand((len(want),) + row + (2,)))
        assert torch.equal(buf.next_state[order], buf.state[order] + 0.5)
        assert torch.equal(buf.action[order], k.to(torch.int64).reshape((-1,) + (1,) * len(row)).expand((len(want),) + row))
        assert torch.equal(buf.reward[order], -buf.action[order].to(torch.float32))
    assert list(want) == [9, 10, 11, 12, 13]


@pytest.mark.parametrize("kind", ["dqn", "maddpg"])
def test_ring_push_batch_and_shape_messages(kind):
    buf, row = _ring(kind)
    T = 2
    shape = (T + 1, 2) + row + (2,)      # [T + 1, A, F] of collect_dqn_transitions, [T + 1, E, N, F] of collect_maddpg_transitions
    states = torch.arange(float(torch.Size(shape).numel())).reshape(shape)
    lead = shape[1:-1]
    batch = {"state": states, "action": torch.ones((T,) + lead, dtype=torch.int64), "reward": torch.zeros((T,) + lead)}
    buf.push_batch(batch)
    n = len(buf)
    assert n == T * lead[0]
    assert torch.equal(buf.state[:n], states[:T].reshape((n,) + row + (2,))) and torch.equal(buf.next_state[:n], states[1:].reshape((n,) + row + (2,)))
    name = "DeviceReplayBuffer" if kind == "dqn" else "JointReplayBuffer"
    with pytest.raises(ValueError, match=name + r"\.push: state / next_state \[n, "):
        buf.push(torch.zeros((1,) + row + (3,)), torch.zeros((1,) + row, dtype=torch.int64), torch.zeros((1,) + row), torch.zeros((1,) + row + (3,)))
    assert len(buf) == n


def test_minibatches_are_what_ppo_learner_cut_before_the_helper_moved():
    """(n = 10, batch_size = 4, seed = 3, epoch = 1) on the CPU: the index tensors ``PPOLearner.minibatches`` returned at the commit
    before this module existed, recorded there."""
    got = L.minibatches(torch.device("cpu"), 10, 4, "torch", 3, 1)
    assert [t.tolist() for t in got] == [[7, 6, 0, 1], [9, 2, 4, 5], [8, 3]]
    assert all(t.dtype == torch.int64 for t in got)
    again = torch.randperm(10, generator=L.seeded_generator(3, 1, "cpu"))
    assert torch.equal(torch.cat(got), again)


def test_validation_messages():
    with pytest.raises(ValueError, match="^backend must be 'auto', 'hip' or 'torch'$"):
        L.check_backend("cuda")
    with pytest.raises(ValueError, match="^critic_backend must be 'auto', 'hip' or 'torch'$"):
        L.check_backend("cuda", "critic_backend")
    assert L.check_sampler(None, graph=True) == "philox" and L.check_sampler(None, graph=False) == "torch"
    with pytest.raises(ValueError, match="^sampler must be 'torch' or 'philox'$"):
        L.check_sampler("numpy", False)
    L.require(None, "PPOLearner")
    with pytest.raises(ValueError, match=r"^TarMACPPOLearner\(critic_backend='hip'\): too wide$"):
        L.require("too wide", "TarMACPPOLearner", "critic_backend")
    assert L.sized(16, "f", "mdr_x_workspace_bytes") == 16
    with pytest.raises(ValueError, match="^f: mdr_x_workspace_bytes refused the sizes$"):
        L.sized(-1, "f", "mdr_x_workspace_bytes")
    fn, name = L.fn(type("lib", (), {"mdr_dqn_grad": 1, "mdr_dqn_grad_wide": 2}), "mdr_dqn_grad", True)
    assert (fn, name) == (2, "mdr_dqn_grad_wide") and L.fn(type("lib", (), {"mdr_dqn_grad": 1}), "mdr_dqn_grad", False) == (1, "mdr_dqn_grad")
