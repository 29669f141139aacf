"""mdr_amd.maddpg's MADDPGLearner, train_maddpg, collect_maddpg_transitions and GreedyDDPGActor on the GPU.

One update() runs 2 N optimiser steps in sequence.  Before the first one both backends hold the same parameters, on the dyadic grids
of tests/maddpg_grad_ref.py: agent 0's critic loss and gradient are held to that file's derived bound against fp64.  Every later
step starts from parameters that already differ by roundings, and Adam's first steps move every element by about lr * sign(g)
whatever the size of g - an element whose gradient is within its own rounding error of zero may move by up to 2 lr the other way.
So the later quantities are compared between the two backends: the losses to 1e-3 (1 + |loss|) (lr-sized parameter steps of which
a rounding-sized share differs), the parameter update p_after - p_before to 1e-2 of its L2 norm (gradient elements are some 1e-3 with
errors of some 1e-9: well under 1e-4 of the elements can flip, each by at most 2 lr against a norm of about lr sqrt(n)) and every
element to the 2 N steps' 2 lr each; both target nets are the blend of their own backend's nets within three roundings."""
import numpy as np
import pytest
import torch

from tests import maddpg_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
N, F_LEN, H, B = 3, 51, 100, 17
LR_A, LR_C, SOFT_TAU, TAU = 1e-3, 3e-3, 0.01, 0.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nets(d, prefixes=("", "c")):
    from mdr_amd.maddpg import DDPGNetworkMLP
    out = []
    for prefix in prefixes:
        Hn, K = d[prefix + "W1"].shape
        net = DDPGNetworkMLP(K, d[prefix + "W3"].shape[0], Hn).to(DEV)
        with torch.no_grad():
            for p, k in zip((t for lin in net.fc for t in (lin.weight, lin.bias)), R.PARAM_NAMES):
                p.copy_(_dev(d[prefix + k]))
        out.append(net)
    return out


def _learner(d, backend, optimizer=torch.optim.Adam):
    from mdr_amd.maddpg import MADDPGLearner
    actor, critic = _nets(d)
    learner = MADDPGLearner(actor, critic, N, LR_A, LR_C, gamma=R.GAMMA, soft_tau=SOFT_TAU, gumbel_tau=TAU, batch_size=B, buffer_capacity=64,
                            backend=backend, optimizer=optimizer)
    tgt_actor, tgt_critic = _nets(d, ("t", "tc"))      # targets of their own, so that a policy net used as a target would show
    learner.tgt_actor.load_state_dict(tgt_actor.state_dict())
    learner.tgt_critic.load_state_dict(tgt_critic.state_dict())
    learner.buffer.push(_dev(d["state"]), _dev(d["action"]), _dev(d["reward"]), _dev(d["next_state"]))
    return learner


def _params(learner):
    return [p for net in (learner.actor, learner.critic, learner.tgt_actor, learner.tgt_critic) for p in net.parameters()]


@pytest.mark.parametrize("fused", [False, True], ids=["adam", "fused_adam"])
def test_one_hip_update_against_the_torch_backend(fused):
    from mdr_amd.optim import FusedAdam
    d = R.inputs(40, N, F_LEN, H, H)
    opt = FusedAdam if fused else torch.optim.Adam
    hip, ref = _learner(d, "hip", opt), _learner(d, "torch", opt)
    assert hip.uses_kernels(B) and not ref.uses_kernels(B)
    before = [p.detach().clone() for p in _params(hip)]
    index, noise_t, noise_a = hip.draws(0)
    i2, n2, n3 = ref.draws(0)
    assert torch.equal(index, i2) and torch.equal(noise_t, n2) and torch.equal(noise_a, n3)      # the same minibatches and noise
    # agent 0's critic step as a case of tests/maddpg_grad_ref.py: the minibatch rows gathered, the learner's own noise
    idx = index[0].cpu().numpy()
    case = dict(d, **{k: d[k][idx] for k in ("state", "next_state", "action", "reward")})
    case["noise_t"] = noise_t[0].cpu().numpy()
    case["noise_a"] = np.repeat(noise_a[0].cpu().numpy()[:, None, :], N, axis=1)
    assert not any(b.any() for b in R._pick_bad(case, TAU))      # no pick of this draw is a matter of rounding
    want, bound = R.evaluate(case, 0, TAU), R.bound(case, 0, TAU)
    seen = {"hip": [], "torch": []}
    for name, lrn in (("hip", hip), ("torch", ref)):
        lrn.before_step = lambda l, which, a, name=name: seen[name].append(
            torch.cat([p.grad.reshape(-1) for p in (l.critic if which == "critic" else l.actor).parameters()]).cpu().numpy())
    out_h, out_t = hip.update(seed=0), ref.update(seed=0)
    assert len(seen["hip"]) == len(seen["torch"]) == 2 * N and hip.training_step == ref.training_step == 1
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
    n_own = len(list(hip.actor.parameters())) + len(list(hip.critic.parameters()))
    for i, (p0, ph, pt) in enumerate(zip(before, _params(hip), _params(ref))):
        lr = (LR_A if i < 6 else LR_C) if i < n_own else 1.0
        dh, dt = (ph.detach() - p0).double(), (pt.detach() - p0).double()
        assert float(dt.abs().max()) > 0      # every tensor moved
        rel = float((dh - dt).norm() / dt.norm())
        print("tensor %2d: |update_hip - update_torch| / |update_torch| = %.2e" % (i, rel))
        assert rel <= 1e-2
        if i < n_own:
            assert float((dh - dt).abs().max()) <= 2 * N * 2 * lr
    for lrn in (hip, ref):      # ddpg.py:167-174 on the backend's own nets
        for tgt, net, off in ((lrn.tgt_actor, lrn.actor, n_own), (lrn.tgt_critic, lrn.critic, n_own + 6)):
            for j, (t, p) in enumerate(zip(tgt.parameters(), net.parameters())):
                t0, p64 = before[off + j].double(), p.detach().double()
                blend = (1 - SOFT_TAU) * t0 + SOFT_TAU * p64
                assert bool(((t.detach().double() - blend).abs() <= 3 * U * ((1 - SOFT_TAU) * t0.abs() + SOFT_TAU * p64.abs())).all())


def test_auto_falls_back_for_an_unsupported_net_and_hip_raises():
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
    torch.manual_seed(0)
    actor, critic = DDPGNetworkMLP(8, 2, 300).to(DEV), DDPGNetworkMLP(2 * 10, 1, 300).to(DEV)
    with pytest.raises(ValueError, match="backend='hip'"):
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=16, backend="hip")
    learner = MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, batch_size=4, buffer_capacity=16, backend="auto")
    assert not learner.uses_kernels(4)
    g = torch.Generator(device=DEV).manual_seed(1)
    learner.buffer.push(torch.randn((8, 2, 8), device=DEV, generator=g), torch.randint(0, 2, (8, 2), device=DEV, generator=g),
                        torch.randn((8, 2), device=DEV, generator=g), torch.randn((8, 2, 8), device=DEV, generator=g))
    a_loss, c_loss = learner.update(seed=0)      # the torch path
    assert bool(torch.isfinite(a_loss).all()) and bool(torch.isfinite(c_loss).all())
    ok = MADDPGLearner(DDPGNetworkMLP(8, 2, 32).to(DEV), DDPGNetworkMLP(2 * 10, 1, 32).to(DEV), 2, 1e-3, 1e-3, buffer_capacity=16, backend="auto")
    assert ok.uses_kernels(4)


@pytest.fixture(scope="module")
def small_env():
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=4, device=DEV, seed=11)
    env.reset(episode=0)
    return env


def test_train_maddpg_runs_the_reference_cadence(small_env):
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner, train_maddpg
    env = small_env
    F_len, n = env.obs_vector_length(), env.nb_houses
    torch.manual_seed(3)
    actor, critic = DDPGNetworkMLP(F_len, 2, 64).to(DEV), DDPGNetworkMLP(n * (F_len + 2), 1, 64).to(DEV)
    learner = MADDPGLearner(actor, critic, n, 1e-3, 3e-3, soft_tau=SOFT_TAU, batch_size=8, buffer_capacity=64, backend="hip")
    before = [p.detach().clone() for p in _params(learner)]
    a_losses, c_losses = train_maddpg(env, learner, 4, update_every=2, random_steps=1, seed=2)
    assert a_losses.shape == (2, n) and c_losses.shape == (2, n) and a_losses.is_cuda      # updates after steps 2 and 4
    assert bool(torch.isfinite(a_losses).all()) and bool(torch.isfinite(c_losses).all()) and learner.training_step == 2
    assert len(learner.buffer) == 4 * env.nb_envs      # one env-step per env and step
    after = _params(learner)
    assert all(not torch.equal(p, q) for p, q in zip(before, after))      # the nets moved, and the targets with them
    # two blends towards nets that 2 n Adam steps of at most 4 lr each (the bias-corrected first steps) moved: the targets stay within
    # soft_tau times that of where they were
    for tgt, lr, off in ((learner.tgt_actor, 1e-3, 12), (learner.tgt_critic, 3e-3, 18)):
        for j, t in enumerate(tgt.parameters()):
            assert float((t.detach() - before[off + j]).abs().max()) <= 2 * SOFT_TAU * (2 * n) * 4 * lr


def test_collect_and_deploy(small_env):
    from mdr_amd.maddpg import DDPGNetworkMLP, GreedyDDPGActor
    from mdr_amd.rollout import collect_maddpg_transitions, deploy_policy
    env = small_env
    F_len, n, E = env.obs_vector_length(), env.nb_houses, env.nb_envs
    torch.manual_seed(4)
    actor = DDPGNetworkMLP(F_len, 2, 64).to(DEV)
    batch = collect_maddpg_transitions(env, actor, 3, random_steps_left=1, seed=5)
    assert batch["state"].shape == (4, E, n, F_len) and batch["action"].shape == (3, E, n) and batch["reward"].shape == (3, E, n)
    assert batch["action"].dtype == torch.int64 and int(batch["action"].min()) >= 0 and int(batch["action"].max()) <= 1
    assert bool(torch.isfinite(batch["state"]).all()) and bool(torch.isfinite(batch["reward"]).all())
    out = deploy_policy(env, GreedyDDPGActor(actor), 3)
    assert set(out) == {"reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"}
    assert out["reward_sum"].shape == (E, n) and bool(torch.isfinite(out["reward_sum"]).all())
