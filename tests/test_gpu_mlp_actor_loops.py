"""FusedMLPActor in the loops that opt into it: collect_maddpg_transitions / train_maddpg with actor_backend="hip" and deploy_policy with
GreedyDDPGActor(backend="hip") or a sampled FusedMLPActor, eager and captured.  3 envs x 20 houses, the reference's 51 features and
its 256-256 actor (DDPGNetworkMLP).

Between the two backends of collect_maddpg_transitions the draw is the same and the probabilities differ by fp32 rounding, so an
action may differ only where the uniform falls within the fp32 contract (1e-5 |p| + 2e-6, tests/actor_ref.py) of the fp64 p0: both
backends are held to the fp64 draw outside that margin on their own stored rows, and to each other wherever their rows are equal."""
import numpy as np
import pytest
import torch

from tests import actor_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, N = 3, 20


def _cfg():
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    return cfg


def _env(**kw):
    import mdr_amd
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(), nb_envs=E, device=DEV, seed=11, **kw)
    env.reset(episode=0)
    return env


def _actor(seed=4):
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(seed)
    actor = DDPGNetworkMLP(51, 2, 256).to(DEV)
    with torch.no_grad():      # spread the probabilities: the default init leaves them all near one value
        actor.fc[2].weight.mul_(8.0)
    return actor


def _weights(actor):
    return tuple(t.detach().cpu().numpy().astype(np.float64) for lin in actor.fc for t in (lin.weight, lin.bias))


def test_collect_maddpg_transitions_acts_through_the_kernel():
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import collect_maddpg_transitions
    actor = _actor()
    env_h, env_t = _env(), _env()
    assert env_h.obs_vector_length() == 51 and env_h.steps_taken == 0
    seed, T = 5, 3
    hip = collect_maddpg_transitions(env_h, actor, T, random_steps_left=1, seed=seed, actor_backend="hip")
    ref = collect_maddpg_transitions(env_t, actor, T, random_steps_left=1, seed=seed, actor_backend="torch")
    assert hip["state"].shape == (T + 1, E, N, 51) and hip["action"].shape == (T, E, N) and hip["action"].dtype == torch.int64
    assert bool(torch.isfinite(hip["state"]).all()) and bool(torch.isfinite(hip["reward"]).all())
    assert torch.equal(hip["state"][0], ref["state"][0])
    assert torch.equal(hip["action"][0], ref["action"][0]), "the random step draws from the same generator under both backends"
    assert torch.equal(hip["state"][1], ref["state"][1])
    fused = FusedMLPActor(actor)
    w = _weights(actor)
    agents = np.arange(E * N, dtype=np.uint64)
    excluded = 0
    for t in (1, 2):      # env.steps_taken was t when step t acted
        again, _ = fused.sample(hip["state"][t].view(E * N, 51), seed, t)
        assert torch.equal(again.to(torch.int64), hip["action"][t].view(-1)), "step %d is not FusedMLPActor.sample on the stored rows" % t
        u = ar.draw_u(agents, seed, t).astype(np.float64)
        for batch in (hip, ref):
            _, p0, _, _ = ar.forward64(*w, batch["state"][t].view(E * N, 51).cpu().numpy())
            clear = np.abs(p0 - u) > ar.CONTRACT[False][0] * np.abs(p0) + ar.CONTRACT[False][1]
            want = np.where(u < p0, 0, 1)
            got = batch["action"][t].view(-1).cpu().numpy()
            assert np.array_equal(got[clear], want[clear]), "step %d: actions off the fp64 draw outside the fp32 contract" % t
            excluded += int((~clear).sum())
            if batch is hip and torch.equal(hip["state"][t], ref["state"][t]):
                assert np.array_equal(got[clear], ref["action"][t].view(-1).cpu().numpy()[clear])
    assert excluded <= 0.01 * 4 * E * N
    assert 0 < int(hip["action"][1:].sum()) < 2 * E * N      # both actions occur: the comparison above compares something
    with pytest.raises(ValueError, match="129"):
        from mdr_amd.rollout import ActorMLP
        collect_maddpg_transitions(env_h, ActorMLP(129, 2, (256, 256)).to(DEV), 1, actor_backend="hip")


def test_train_maddpg_acts_through_the_kernel():
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner, train_maddpg
    env = _env()
    torch.manual_seed(3)
    actor, critic = DDPGNetworkMLP(51, 2, 256).to(DEV), DDPGNetworkMLP(N * 53, 1, 256).to(DEV)
    learner = MADDPGLearner(actor, critic, N, 1e-3, 3e-3, batch_size=8, buffer_capacity=64, backend="hip")
    before = [p.detach().clone() for p in actor.parameters()]
    a_losses, c_losses = train_maddpg(env, learner, 4, update_every=4, random_steps=1, seed=2, actor_backend="hip")
    assert a_losses.shape == (1, N) and c_losses.shape == (1, N) and learner.training_step == 1
    assert bool(torch.isfinite(a_losses).all()) and bool(torch.isfinite(c_losses).all())
    assert len(learner.buffer) == 4 * E and env.steps_taken == 4
    assert all(not torch.equal(p, q) for p, q in zip(before, actor.parameters()))


def test_deploy_policy_takes_the_greedy_kernel():
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.rollout import deploy_policy
    actor = _actor()
    out = deploy_policy(_env(), GreedyDDPGActor(actor, backend="hip"), 3)
    assert set(out) == {"reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"}
    assert out["reward_sum"].shape == (E, N) and all(bool(torch.isfinite(v).all()) for v in out.values())
    # the torch form of the same agent: the same argmax wherever the logits are not within rounding of a tie - on 3 steps of 60 agents,
    # the same metrics unless such a tie occurs, so only their shapes are compared
    ref = deploy_policy(_env(), GreedyDDPGActor(actor), 3)
    assert all(out[k].shape == ref[k].shape for k in out)


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_captured_deployment_equals_the_eager_one(greedy):
    """table_steps = 16 and 40 steps: the replays cross two table refills; the sampled form draws by step_dev."""
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import deploy_policy
    actor = _actor()
    T = 40
    envs = [_env(table_steps=16, graph_mode=True), _env(table_steps=16, graph_mode=True), _env(table_steps=16)]
    res = []
    for env, use_graph in zip(envs, (True, False, None)):
        policy = GreedyDDPGActor(actor, backend="hip") if greedy else FusedMLPActor(actor)
        res.append(deploy_policy(env, policy, T, seed=4, use_graph=use_graph))
    for env in envs:
        assert env.steps_taken == T
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]) and torch.equal(res[0][k], res[2][k]), k
    for k in ("Ta", "sso", "reward"):
        assert torch.equal(envs[0].t[k], envs[2].t[k]), k
    if not greedy:      # the draws moved with the device-side step: a frozen step would repeat one step's uniforms 40 times
        frozen = deploy_policy(_env(table_steps=16), _FrozenStep(FusedMLPActor(actor)), T, seed=4)
        assert not torch.equal(frozen["reward_sum"], res[0]["reward_sum"])


class _FrozenStep:
    """A sampled FusedMLPActor that always draws with step 0 - what a captured step without step_dev would do."""

    def __init__(self, fused):
        self.fused = fused

    def sample(self, rows, seed, step, action=None, step_dev=None):
        return self.fused.sample(rows, seed, 0, action=action)
