"""MADDPGLearner(shared=False) - one actor, critic and target of each per agent - on backend="hip" against backend="torch", by the rules
of tests/test_gpu_maddpg_learner.py: the same draws; agent 0's critic loss and gradient to the derived bound of the fp64 restatement
(tests/maddpg_grad_ref.py with agent 0's own nets; every agent's pick from its own target actor, tests/maddpg_agents_ref.py); the
losses to 1e-3 (1 + |loss|); every tensor's update to 1e-2 of its norm and, per element, to 2 lr - an unshared net takes ONE step per
update (the shared nets take N), and Adam's first step moves an element by about lr sign(g), so an element whose gradient is within its
rounding error of zero may move by up to 2 lr the other way.  Then what only the unshared update can get wrong: every agent reads the
target actors as the PREVIOUS update left them (a FusedAdam's blend must not ride on an actor's step), every target is the blend of
its own pair, nets that were equal differ afterwards.  And the loops: train_maddpg and deploy_policy with a list of actors."""
import numpy as np
import pytest
import torch

from tests import maddpg_agents_ref as A
from tests import maddpg_grad_ref as R
from tests.test_gpu_maddpg_learner import B, DEV, F_LEN, H, LR_A, LR_C, N, SOFT_TAU, TAU, U, _dev

pytestmark = pytest.mark.gpu


def _net(params, K, O, Hn):
    from mdr_amd.maddpg import DDPGNetworkMLP
    net = DDPGNetworkMLP(K, O, Hn).to(DEV)
    with torch.no_grad():
        for p, k in zip((t for lin in net.fc for t in (lin.weight, lin.bias)), R.PARAM_NAMES):
            p.copy_(_dev(params[k]))
    return net


def _case_nets(d, equal=False):
    """Per agent: actor, critic, target actor, target critic.  Agent 0's are the shared case's four nets; agent k's actor and target
    actor are maddpg_agents_ref's net k and, for the actor, another agent's net of that set; the critics are agent 0's scaled by
    1 + k / 8 in their last layer (a dyadic factor: the grids stay exact)."""
    tgt = A.target_actors(N, F_LEN, H, H, equal)
    J = N * (F_LEN + 2)
    out = []
    for k in range(N):
        j = 0 if equal else k
        actor = {n: (d[n] if j == 0 else tgt[(j + 1) % N if (j + 1) % N else 1][n]) for n in R.PARAM_NAMES}
        scale = np.float32(1 + j / 8)
        critic = {n: (d["c" + n] * scale if n in ("W3", "b3") else d["c" + n]) for n in R.PARAM_NAMES}
        tcritic = {n: (d["tc" + n] * scale if n in ("W3", "b3") else d["tc" + n]) for n in R.PARAM_NAMES}
        out.append((_net(actor, F_LEN, 2, H), _net(critic, J, 1, H), _net(tgt[j], F_LEN, 2, H), _net(tcritic, J, 1, H)))
    return out


def _learner(d, backend, optimizer=torch.optim.Adam, equal=False):
    from mdr_amd.maddpg import MADDPGLearner
    nets = _case_nets(d, equal)
    learner = MADDPGLearner([n[0] for n in nets], [n[1] for n in nets], N, LR_A, LR_C, gamma=R.GAMMA, soft_tau=SOFT_TAU, gumbel_tau=TAU,
                            batch_size=B, buffer_capacity=64, backend=backend, optimizer=optimizer, shared=False)
    for k in range(N):
        learner.tgt_actors[k].load_state_dict(nets[k][2].state_dict())
        learner.tgt_critics[k].load_state_dict(nets[k][3].state_dict())
    learner.buffer.push(_dev(d["state"]), _dev(d["action"]), _dev(d["reward"]), _dev(d["next_state"]))
    return learner


def _params(learner):
    groups = (learner.actors, learner.critics, learner.tgt_actors, learner.tgt_critics)
    return [p for nets in groups for net in nets for p in net.parameters()]


@pytest.mark.parametrize("fused", [False, True], ids=["adam", "fused_adam"])
def test_one_unshared_hip_update_against_the_torch_backend(fused):
    from mdr_amd.optim import FusedAdam
    d = R.inputs(40, N, F_LEN, H, H)
    opt = FusedAdam if fused else torch.optim.Adam
    hip, ref = _learner(d, "hip", opt), _learner(d, "torch", opt)
    assert hip.uses_kernels(B) and not ref.uses_kernels(B) and not hip.shared
    before = [p.detach().clone() for p in _params(hip)]
    draws_h, draws_t = hip.draws(0), ref.draws(0)
    assert all(torch.equal(x, y) for x, y in zip(draws_h, draws_t))      # the same minibatches and noise
    index, noise_t, noise_a = draws_h
    # agent 0's critic step as a case of the restatements: the minibatch rows gathered, the learner's own noise and nets
    idx = index[0].cpu().numpy()
    case = dict(d, **{k: d[k][idx] for k in ("state", "next_state", "action", "reward")})
    case["noise_t"] = noise_t[0].cpu().numpy()
    case["noise_a"] = np.repeat(noise_a[0].cpu().numpy()[:, None, :], N, axis=1)
    tgt_nets = A.target_actors(N, F_LEN, H, H)
    assert not A.pick_bad(case, tgt_nets, TAU).any()      # no pick of this draw is a matter of rounding
    picks = A.picks(case, tgt_nets, TAU)
    want_t, bound_t = A.evaluate(case, tgt_nets, 0, TAU), A.bound(case, tgt_nets, 0, TAU)
    # the critic's loss and gradient follow from y: maddpg_grad_ref on a case whose shared target actor gives these very picks is not
    # available, so the bound of the mse step is taken with the per-agent y: E_y enters maddpg_grad_ref.bound through its own target
    # part only, which depends on the picks through next_action alone - evaluate both with the picks forced
    forced = dict(case, noise_t=np.where(picks[:, :, None] == np.array([0, 1])[None, None, :], 1e6, -1e6).astype(np.float32))
    want, bound = R.evaluate(forced, 0, TAU), R.bound(forced, 0, TAU)
    assert np.array_equal(want["next_action"], picks) and np.array_equal(want["y"], want_t["y"]) and np.allclose(bound["y"], bound_t["y"], rtol=1e-12)
    seen = {"hip": [], "torch": []}
    tgts = {"hip": [], "torch": []}

    def hook(name):
        def record(l, which, a):
            net = (l.critics if which == "critic" else l.actors)[a]
            seen[name].append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu().numpy())
            tgts[name].append([p.detach().clone() for t in l.tgt_actors for p in t.parameters()])
        return record

    hip.before_step, ref.before_step = hook("hip"), hook("torch")
    out_h, out_t = hip.update(seed=0), ref.update(seed=0)
    assert len(seen["hip"]) == len(seen["torch"]) == 2 * N and hip.training_step == ref.training_step == 1
    n_a = 6 * N
    for name in ("hip", "torch"):      # all 2 N calls saw the target actors of before the update: no blend rode on an actor's step
        for snap in tgts[name]:
            assert all(torch.equal(x, y) for x, y in zip(snap, before[2 * n_a:3 * n_a])), name
    for name, out in (("hip", out_h), ("torch", out_t)):
        w_grad = R.worst(seen[name][0], want["cgrad"], bound["cgrad"])
        w_loss = R.worst(float(out[1][0]), want["closs"], bound["closs"])
        print("%s: agent 0's critic step, worst |error| / bound: grad %.3f, loss %.3f" % (name, w_grad, w_loss))
        assert w_grad <= 1.0 and w_loss <= 1.0
    for k in (0, 1):
        assert out_h[k].shape == (N,) and out_h[k].is_cuda and bool(torch.isfinite(out_h[k]).all())
        off = float(((out_h[k] - out_t[k]).abs() / (1 + out_t[k].abs())).max())
        print("%s losses: max |hip - torch| / (1 + |torch|) = %.2e" % (("actor", "critic")[k], off))
        assert off <= 1e-3
    after_h, after_t = _params(hip), _params(ref)
    for i, (p0, ph, pt) in enumerate(zip(before, after_h, after_t)):
        dh, dt = (ph.detach() - p0).double(), (pt.detach() - p0).double()
        assert float(dt.abs().max()) > 0      # every tensor moved
        rel = float((dh - dt).norm() / dt.norm())
        print("tensor %2d: |update_hip - update_torch| / |update_torch| = %.2e" % (i, rel))
        assert rel <= 1e-2
        if i < 2 * n_a:      # the trained nets: ONE Adam step each
            assert float((dh - dt).abs().max()) <= 2 * (LR_A if i < n_a else LR_C)
    for after in (after_h, after_t):      # ddpg.py:167-174: every target the blend of its own pair, on the backend's own nets
        for j in range(2 * n_a):
            t0, p64 = before[2 * n_a + j].double(), after[j].detach().double()
            blend = (1 - SOFT_TAU) * t0 + SOFT_TAU * p64
            assert bool(((after[2 * n_a + j].detach().double() - blend).abs() <= 3 * U * ((1 - SOFT_TAU) * t0.abs() + SOFT_TAU * p64.abs())).all()), j


def test_equal_nets_differ_after_the_update_and_the_checkpoint_round_trips():
    d = R.inputs(40, N, F_LEN, H, H)
    hip = _learner(d, "hip", equal=True)
    assert all(torch.equal(x, y) for x, y in zip(hip.actors[0].parameters(), hip.actors[1].parameters()))
    hip.update(seed=0)
    for nets in (hip.actors, hip.critics):      # each agent trained on its own minibatch
        assert not torch.equal(nets[0].fc[0].weight, nets[1].fc[0].weight) and not torch.equal(nets[1].fc[2].weight, nets[2].fc[2].weight)
    fresh = _learner(d, "hip")
    fresh.load_network_dict(hip.network_dict())
    fresh.training_step = hip.training_step
    for x, y in zip(hip.update(seed=1), fresh.update(seed=1)):
        assert torch.equal(x, y)
    for x, y in zip(_params(hip), _params(fresh)):
        assert torch.equal(x, y)


def test_shared_mode_keeps_its_bits_beside_the_unshared_one():
    from tests.test_gpu_maddpg_learner import _learner as shared_learner
    d = R.inputs(40, N, F_LEN, H, H)
    one, two = shared_learner(d, "hip"), shared_learner(d, "hip")
    assert one.shared and all(m is one.actor for m in one.actors) and all(o is one.actor_optimizer for o in one.actor_optimizers)
    _learner(d, "hip").update(seed=0)      # an unshared learner in between leaves no state behind
    for x, y in zip(one.update(seed=0), two.update(seed=0)):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def small_cfg():
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    return cfg


def _env(cfg, **kw):
    import mdr_amd
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=4, device=DEV, seed=11, **kw)
    env.reset(episode=0)
    return env


def _twenty(seed=0):
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(seed)
    n, f = 20, 51
    return [DDPGNetworkMLP(f, 2, 64).to(DEV) for _ in range(n)], [DDPGNetworkMLP(n * (f + 2), 1, 64).to(DEV) for _ in range(n)]


@pytest.mark.parametrize("actor_backend", ["torch", "hip"])
def test_train_maddpg_with_twenty_agents_nets(small_cfg, actor_backend):
    from mdr_amd.maddpg import MADDPGLearner, train_maddpg
    actors, critics = _twenty()
    learner = MADDPGLearner(actors, critics, 20, 1e-3, 3e-3, batch_size=8, buffer_capacity=64, backend="hip", shared=False)
    before = [a.fc[0].weight.detach().clone() for a in actors]
    a_losses, c_losses = train_maddpg(_env(small_cfg), learner, 4, update_every=2, random_steps=1, seed=2, actor_backend=actor_backend)
    assert a_losses.shape == (2, 20) and c_losses.shape == (2, 20)
    assert bool(torch.isfinite(a_losses).all()) and bool(torch.isfinite(c_losses).all())
    assert all(not torch.equal(a.fc[0].weight, w) for a, w in zip(actors, before))      # all 20 actors moved


def test_both_actor_backends_take_the_same_actions(small_cfg):
    """tests/test_gpu_mlp_actor_loops.py's rule: the probabilities to fp32 rounding, the actions wherever |u - p0| exceeds it."""
    from mdr_amd.mlp_actor import FusedMLPActors
    from mdr_amd.rollout import collect_maddpg_transitions
    from tests import actor_ref as ar
    actors, _ = _twenty()
    got = {k: collect_maddpg_transitions(_env(small_cfg), actors, 1, seed=5, actor_backend=k) for k in ("torch", "hip")}
    assert torch.equal(got["torch"]["state"][0], got["hip"]["state"][0])
    rows = got["hip"]["state"][0].reshape(80, 51)
    _, _, probs = FusedMLPActors(actors).sample(rows, 5, 0, want_probs=True)
    with torch.no_grad():
        ref = torch.stack([actors[k](got["hip"]["state"][0][:, k]) for k in range(20)], 1).reshape(80, 2).softmax(-1)
    tol = 1e-5 * ref + 2e-6
    assert bool(((probs - ref).abs() <= tol).all())
    u = torch.from_numpy(ar.draw_u(np.arange(80, dtype=np.uint64), 5, 0)).to(DEV)
    clear = (u - ref[:, 0]).abs() > tol[:, 0]
    a_t, a_h = got["torch"]["action"].reshape(80), got["hip"]["action"].reshape(80)
    assert int(clear.sum()) >= 70 and torch.equal(a_t[clear], a_h[clear])


def test_deploy_policy_eager_and_captured(small_cfg):
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.rollout import deploy_policy
    actors, _ = _twenty()
    res = [deploy_policy(_env(small_cfg, table_steps=16, graph_mode=True), GreedyDDPGActor(actors, backend="hip"), 20, seed=4, use_graph=g)
           for g in (False, True)]
    assert set(res[0]) == set(res[1])
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    ref = deploy_policy(_env(small_cfg, table_steps=16), GreedyDDPGActor(actors), 20, seed=4)      # N torch forwards: the same shapes
    assert all(ref[k].shape == res[0][k].shape for k in res[0])
