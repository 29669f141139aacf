"""mdr_amd.dqn's replay buffer, DQNLearner and train_dqn on the GPU, on transitions collect_dqn_transitions leaves on the device:
4 envs x 20 houses x 8 steps = 640 transitions into a buffer of 512."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
CAPACITY, BATCH = 512, 256


def _net(F, seed):
    from mdr_amd.dqn import QNetworkMLP
    torch.manual_seed(seed)
    return QNetworkMLP(F).to(DEV)


def _clone(net):
    """A fresh module with the same parameters (collect_dqn_transitions leaves its packed kernel operands on the network: no deepcopy)."""
    twin = type(net)(net.fc[0].in_features, 2, net.layers)
    twin.load_state_dict(net.state_dict())
    return twin.to(DEV)


@pytest.fixture(scope="module")
def collected():
    import mdr_amd
    from mdr_amd.rollout import collect_dqn_transitions
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=4, device=DEV, seed=11)
    env.reset(episode=0)
    net = _net(env.obs_vector_length(), 1)
    batch = collect_dqn_transitions(env, net, 8, epsilon=0.5, seed=3)
    assert batch["reward"].numel() == 640
    return env, net, batch


def _learner(net, **kw):
    from mdr_amd.dqn import DQNLearner
    kw.setdefault("buffer_capacity", CAPACITY)
    kw.setdefault("batch_size", BATCH)
    return DQNLearner(_clone(net), 1e-3, **kw)


def _steps(batch, lo, hi):
    return dict(state=batch["state"][lo:hi + 1], action=batch["action"][lo:hi], reward=batch["reward"][lo:hi])


def _flat(batch):
    s = batch["state"]
    return s[:-1].reshape(-1, s.shape[-1]), batch["action"].reshape(-1), batch["reward"].reshape(-1), s[1:].reshape(-1, s.shape[-1])


def test_store_keeps_the_last_512_transitions_in_ring_order(collected):
    _, net, batch = collected
    want = [t[-CAPACITY:] for t in _flat(batch)]
    whole, pieces = _learner(net, backend="torch"), _learner(net, backend="torch")
    whole.store(batch)                      # one push larger than the buffer: its tail stays
    pieces.store(_steps(batch, 0, 5))       # 400 rows, then 240 across the wrap
    pieces.store(_steps(batch, 5, 8))
    assert pieces.buffer._pos == 128
    for lrn in (whole, pieces):
        buf = lrn.buffer
        assert len(buf) == CAPACITY
        order = buf.chronological()
        for got, ref in zip((buf.state, buf.action, buf.reward, buf.next_state), want):
            assert torch.equal(got[order], ref)


def test_both_backends_draw_the_same_indices(collected):
    _, net, batch = collected
    a, b = _learner(net, backend="hip"), _learner(net, backend="torch")
    a.store(batch), b.store(batch)
    for seed in (0, 7):
        i, j = a.sample(seed), b.sample(seed)
        assert i.dtype == torch.int64 and i.shape == (BATCH,) and torch.equal(i, j)
        assert int(i.min()) >= 0 and int(i.max()) < CAPACITY
    assert not torch.equal(a.sample(0), a.sample(7))


def _fp64_gradient(policy, target, buf, index, gamma, double):
    """agents/dqn.py:93-109 on the minibatch in fp64 (DDQN with the per-row target) -> the six clamped gradients."""
    p64, t64 = _clone(policy).double(), _clone(target).double()
    s, a, r, sn = buf.state[index].double(), buf.action[index].view(-1, 1), buf.reward[index].double().view(-1, 1), buf.next_state[index].double()
    with torch.no_grad():
        nq = t64(sn).gather(1, p64(sn).argmax(1, keepdim=True)) if double else t64(sn).max(1)[0].unsqueeze(1)
    loss = torch.nn.SmoothL1Loss()(p64(s).gather(1, a), r + nq * gamma)
    loss.backward()
    return [p.grad.clamp(-1, 1) for p in p64.parameters()]


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
def test_first_hip_update_takes_the_gradient_of_the_direct_calls(collected, double):
    """(a) bit for bit what td_target + q_loss_backward give; (b) the reference's expression in fp64 - with a target net that is NOT
    the policy net's copy, so that DDQN's pick and DQN's maximum differ, and the rewards scaled by 1 / 64 into the quadratic part of
    the Huber loss, where the gradient follows the target - to 1e-3 of each parameter's largest gradient element (fp32 sums of 256
    rows through three layers are some (256 + 100) u = 2e-5 of it off; a next-state row whose two policy Q-values tie within
    rounding may flip its pick and move the gradient by its share, under 1 / 256 of it), which the other mode's gradient is not."""
    from mdr_amd import dqn
    _, net, batch = collected
    learner = _learner(net, backend="hip", double=double)
    learner.target_net.load_state_dict(_net(net.fc[0].in_features, 99).state_dict())
    learner.store(batch)
    learner.buffer.reward.mul_(1.0 / 64)
    idx = learner.sample(0)
    twin, target = _clone(learner.policy_net), _clone(learner.target_net)
    y, _, _ = dqn.td_target(target, learner.buffer.next_state, learner.buffer.reward, learner.gamma, index=idx, policy_net=twin if double else None)
    dqn.q_loss_backward(twin, learner.buffer.state, learner.buffer.action, y, index=idx, grad_clamp=1.0)
    mine = _fp64_gradient(learner.policy_net, learner.target_net, learner.buffer, idx, learner.gamma, double)
    other = _fp64_gradient(learner.policy_net, learner.target_net, learner.buffer, idx, learner.gamma, not double)
    seen = []
    learner.before_step = lambda lrn: seen.append([p.grad.clone() for p in lrn.policy_net.parameters()])
    loss = learner.update(seed=0)
    assert loss.is_cuda and loss.dim() == 0 and len(seen) == 1 and learner.training_step == 1
    for g, p in zip(seen[0], twin.parameters()):
        assert torch.equal(g, p.grad)
    off_mine = max(float((g.double() - m).abs().max() / m.abs().max()) for g, m in zip(seen[0], mine))
    off_other = max(float((g.double() - o).abs().max() / o.abs().max()) for g, o in zip(seen[0], other))
    print("double=%s: |hip - fp64| / max|fp64| = %.2e (own mode), %.2e (the other mode)" % (double, off_mine, off_other))
    assert off_mine < 1e-3 < off_other


def _fp64_td_loss(policy, target, buf, gamma):
    """The Huber TD loss of agents/dqn.py:93-103 over the whole buffer in fp64."""
    p64, t64 = _clone(policy).double(), _clone(target).double()
    with torch.no_grad():
        y = buf.reward.double().view(-1, 1) + t64(buf.next_state.double()).max(1)[0].unsqueeze(1) * gamma
        return float(torch.nn.SmoothL1Loss()(p64(buf.state.double()).gather(1, buf.action.view(-1, 1)), y))


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_twenty_updates_against_a_fixed_target_lower_the_td_loss(collected, backend):
    _, net, batch = collected
    learner = _learner(net, backend=backend, tau=0.0)
    frozen = _clone(learner.target_net)
    assert learner.update() is None      # fewer transitions than a minibatch: agents/dqn.py:85-86
    learner.store(batch)
    before = _fp64_td_loss(learner.policy_net, frozen, learner.buffer, learner.gamma)
    losses = [learner.update(seed=0) for _ in range(20)]
    after = _fp64_td_loss(learner.policy_net, frozen, learner.buffer, learner.gamma)
    print("%s: fp64 Huber TD loss over the buffer %.6f -> %.6f" % (backend, before, after))
    assert all(bool(torch.isfinite(l)) for l in losses) and learner.training_step == 20
    for p, q in zip(learner.target_net.parameters(), frozen.parameters()):
        assert torch.equal(p, q)         # tau = 0: the blend leaves the target where it was
    assert after < before
    assert all(bool(torch.isfinite(p).all()) for p in learner.policy_net.parameters())


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_soft_update_blends_within_three_roundings(collected, backend):
    _, net, batch = collected
    learner = _learner(net, backend=backend, tau=0.01)
    learner.store(batch)
    old = [p.detach().double().clone() for p in learner.target_net.parameters()]
    learner.update(seed=0)
    for t, t0, p in zip(learner.target_net.parameters(), old, learner.policy_net.parameters()):
        assert not torch.equal(p.detach().double(), t0)      # the optimiser moved the policy net
        want = 0.99 * t0 + 0.01 * p.detach().double()
        bound = 3 * U * (0.99 * t0.abs() + 0.01 * p.detach().double().abs())
        assert bool(((t.detach().double() - want).abs() <= bound).all())
    still = _learner(net, backend=backend, tau=0.01, double=True, soft_update=False)      # the reference's DDQN never blends
    still.store(batch)
    old = [p.detach().clone() for p in still.target_net.parameters()]
    still.update(seed=0)
    assert all(torch.equal(t, t0) for t, t0 in zip(still.target_net.parameters(), old))


def test_the_trained_network_deploys_and_train_dqn_runs(collected):
    from mdr_amd import dqn
    from mdr_amd.policy import FusedActor
    from mdr_amd.rollout import deploy_policy
    env, net, batch = collected
    learner = _learner(net, backend="hip")
    learner.store(batch)
    losses, eps = dqn.train_dqn(env, learner, 3, updates_per_step=2, epsilon=0.5, epsilon_decay=0.9, min_epsilon=0.1, seed=2)
    assert losses.shape == (6,) and losses.is_cuda and bool(torch.isfinite(losses).all())
    assert abs(eps - 0.5 * 0.9 ** 3) < 1e-12 and learner.training_step == 6 and len(learner.buffer) == CAPACITY
    out = deploy_policy(env, FusedActor.from_module(learner.policy_net, greedy=True), 4, greedy=True)
    assert bool(torch.isfinite(out["reward_sum"]).all())
