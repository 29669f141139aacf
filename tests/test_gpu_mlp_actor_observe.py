"""Observe -> act for the 256-unit fused actor: FusedMLPActor.sample_env / mdr_env_mlp_actor_sample[_bf16x3]
(csrc/mdr_mlp_actor_observe.hip) against the rows path it replaces, FusedMLPActor.sample(env.obs_vector("rows").view(E * N, 51), ...).
No tolerances: the staged features are the rows' bits and the matrix instructions take them in the same order, so every output is
compared with torch.equal; the rows path itself is held to the fp64 forward by tests/test_gpu_mlp_actor.py and
tests/test_gpu_mlp_actor_bf16.py."""
import ctypes as C

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = ["fp32", "bf16x3"]
BACKENDS = {"fp32": "hip", "bf16x3": "hip-bf16x3"}
ENTRIES = {"fp32": "mdr_env_mlp_actor_sample", "bf16x3": "mdr_env_mlp_actor_sample_bf16x3"}
# (3, 11): the smallest env, its window wraps onto the whole env, A = 33 ends in a partial tile; (7, 20): tiles that span envs;
# (4, 32): whole-env tiles (the aligned staging); (2, 300), (1, 1024): tiles inside a large env, halos that wrap at its ends
SHAPES = [(3, 11), (7, 20), (5, 50), (4, 32), (2, 300), (1, 1024)]


def _cfg(N, **patches):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["default_env_prop"]["power_grid_prop"]["signal_mode"] = "perlin"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    cfg["default_hvac_prop"]["lockout_noise"] = 15
    for dotted, v in patches.items():
        node = cfg
        parts = dotted.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


def _walk(env, steps, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(steps):
        env.step((torch.rand((env.nb_envs, env.nb_houses), generator=g) < 0.5).to(torch.uint8).to(DEV))


_ENVS = {}


def _env(E, N):
    """An env a dozen random steps into its episode - lockouts, seconds_since_off and on / off flags mixed - built once per shape
    and never stepped again: sampling does not change it."""
    import mdr_amd
    if (E, N) not in _ENVS:
        env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device=DEV, seed=5 + N)
        env.reset(episode=0)
        _walk(env, 12, seed=N)
        _ENVS[(E, N)] = env
    return _ENVS[(E, N)]


def _fresh(E, N, patches=None, **kw):
    import mdr_amd
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N, **(patches or {})), nb_envs=E, device=DEV, seed=4, **kw)
    env.reset(episode=0)
    return env


class _Net(nn.Module):
    """Linear - ReLU - Linear - ReLU - Linear with two hidden sizes of its own, held as `fc`."""

    def __init__(self, F, H1, H2):
        super().__init__()
        self.fc = nn.ModuleList([nn.Linear(F, H1), nn.Linear(H1, H2), nn.Linear(H2, 2)])
        for lin in self.fc:      # as DDPGNetworkMLP
            nn.init.xavier_uniform_(lin.weight, gain=nn.init.calculate_gain("relu"))
            lin.bias.data.fill_(0.01)

    def forward(self, x):
        return self.fc[2](torch.relu(self.fc[1](torch.relu(self.fc[0](x)))))


def _actor(F=51, hidden=256, seed=11):
    """MADDPG's actor with the head's weights times 8, so that p0 spreads over (0, 1), and the head's bias moved so that the logit
    difference has its median at 0 on the rows of the (5, 50) env (the hidden units are non-negative: without that the difference
    sits far on one side and every probability is 0 or 1); `hidden` = (H1, H2): another shape."""
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(seed)
    actor = DDPGNetworkMLP(F, 2, hidden) if isinstance(hidden, int) else _Net(F, *hidden)
    actor = actor.to(DEV)
    with torch.no_grad():
        actor.fc[2].weight.mul_(8.0)
        if F == 51:
            logits = actor(_rows(_env(5, 50)))
            actor.fc[2].bias[0] -= (logits[:, 0] - logits[:, 1]).median()
    return actor


def _fused(actor, precision, **kw):
    from mdr_amd.mlp_actor import FusedMLPActor
    return FusedMLPActor(actor, precision=precision, **kw)


def _rows(env):
    return env.obs_vector("rows").view(env.nb_envs * env.nb_houses, 51)


def _both(fused, env, seed=9, step=4, env_kw=None, **kw):
    by_rows = fused.sample(_rows(env), seed, step, want_probs=True, **kw)
    by_state = fused.sample_env(env, seed, step, want_probs=True, **kw, **(env_kw or {}))
    return by_rows, by_state


def _assert_equal(a, b, what):
    for name, x, y in zip(("action", "a_prob", "probs"), a, b):
        assert x.shape == y.shape and torch.equal(x, y), "%s: %s differs" % (what, name)
    assert bool(torch.isfinite(b[2]).all()), what


def _assert_spread(probs, what):
    p0 = probs[:, 0]
    assert 0.02 < float(p0.mean()) < 0.98 and float(p0.std()) > 0.01, "%s: a saturated actor" % what


@pytest.mark.parametrize("hidden", [256, (100, 60)], ids=["256-256", "100-60"])      # 100-60: the skipped-block branches
@pytest.mark.parametrize("greedy", [False, True], ids=["drawn", "greedy"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sample_env_equals_sample_on_the_rows(precision, greedy, hidden):
    fused = _fused(_actor(hidden=hidden), precision)
    step_dev = torch.tensor([5], dtype=torch.int32, device=DEV)
    spread = []
    for E, N in SHAPES:
        env = _env(E, N)
        what = "%s E%d N%d" % (precision, E, N)
        assert fused.observe_supported(env), what
        by_rows, by_state = _both(fused, env, greedy=greedy)
        _assert_equal(by_rows, by_state, what)
        spread.append(by_state[2])
        # a device word of 5 on top of step 7 is step 12
        moved = fused.sample_env(env, 9, 7, step_dev=step_dev, greedy=greedy, want_probs=True)
        _assert_equal(fused.sample(_rows(env), 9, 12, greedy=greedy, want_probs=True), moved, what + " step_dev")
        if not greedy and E * N >= 250:
            assert not torch.equal(moved[0], by_state[0]), what + ": the draw does not depend on the step"
    _assert_spread(torch.cat(spread), precision)
    if greedy:
        assert 0 < int(torch.cat(spread)[:, 0].ge(0.5).sum()) < sum(E * N for E, N in SHAPES)


@pytest.mark.parametrize("shape", [(5, 50), (7, 20)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_outputs_do_not_depend_on_the_grid(precision, shape):
    """max_workgroups = 1: one workgroup restages its window for every tile (8 and 5 of them)."""
    env = _env(*shape)
    fused = _fused(_actor(), precision)
    A = shape[0] * shape[1]
    reference = fused.sample(_rows(env), 9, 4, want_probs=True)
    for mw in (1, 3, 0):
        rows_out = torch.empty((A, 51), device=DEV)
        _assert_equal(reference, fused.sample_env(env, 9, 4, want_probs=True, max_workgroups=mw), "%s mw %d" % (precision, mw))
        _assert_equal(reference, fused.sample_env(env, 9, 4, want_probs=True, max_workgroups=mw, rows_out=rows_out), "%s mw %d kept" % (precision, mw))
        assert torch.equal(rows_out, _rows(env)), "rows_out with max_workgroups = %d" % mw


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_out_is_obs_vector_rows_and_nothing_else_is_written(precision):
    fused = _fused(_actor(), precision)
    nan = float("nan")
    for E, N in SHAPES:
        env = _env(E, N)
        A = E * N
        what = "%s E%d N%d" % (precision, E, N)
        before = _rows(env).clone()
        plain = fused.sample_env(env, 9, 4, want_probs=True)
        # every output inside a larger canary-filled buffer: 3 floats / 5 bytes in front (rows_out then starts 12 bytes off a 16-byte boundary)
        wide = torch.full((3 + A * 51 + 7,), nan, device=DEV)
        act_buf = torch.full((5 + A + 9,), 0xEE, dtype=torch.uint8, device=DEV)
        prob_buf = torch.full((3 + A + 5,), nan, device=DEV)
        kept = fused.sample_env(env, 9, 4, want_probs=True, rows_out=wide[3:3 + A * 51], action=act_buf[5:5 + A], a_prob=prob_buf[3:3 + A])
        assert torch.equal(wide[3:3 + A * 51].view(A, 51), before), what + ": rows_out differs from obs_vector('rows')"
        assert bool(torch.isnan(wide[:3]).all()) and bool(torch.isnan(wide[3 + A * 51:]).all()), what
        assert bool((act_buf[:5] == 0xEE).all()) and bool((act_buf[5 + A:] == 0xEE).all()), what
        assert bool(torch.isnan(prob_buf[:3]).all()) and bool(torch.isnan(prob_buf[3 + A:]).all()), what
        assert kept[0].data_ptr() == act_buf[5:].data_ptr() and kept[1].data_ptr() == prob_buf[3:].data_ptr()
        _assert_equal(plain, kept, what + " with rows_out")
        # a 16-byte aligned rows_out: the vector stores
        aligned = torch.full((A * 51 + 8,), nan, device=DEV)
        fused.sample_env(env, 9, 4, rows_out=aligned[:A * 51])
        assert torch.equal(aligned[:A * 51].view(A, 51), before) and bool(torch.isnan(aligned[A * 51:]).all()), what + ": aligned rows_out"
        # sampling does not change the env
        assert torch.equal(_rows(env), before), what + ": the env changed"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_weights_are_read_in_place(precision):
    env = _env(5, 50)
    actor = _actor()
    fused = _fused(actor, precision)
    first = fused.sample_env(env, 9, 4, want_probs=True)
    with torch.no_grad():
        actor.fc[1].weight.mul_(0.5)
    second = fused.sample_env(env, 9, 4, want_probs=True)
    _assert_equal(fused.sample(_rows(env), 9, 4, want_probs=True), second, precision)
    assert not torch.equal(first[2], second[2])


def test_sample_env_allocates_nothing_with_its_outputs_given():
    env = _env(5, 50)
    A = 250
    for precision in PRECISIONS:
        fused = _fused(_actor(), precision)
        action = torch.empty(A, dtype=torch.uint8, device=DEV)
        a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
        rows = torch.empty((A, 51), device=DEV)
        fused.sample_env(env, 1, 0, action=action, a_prob=a_prob, rows_out=rows)
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        for t in range(3):
            fused.sample_env(env, 1, t, action=action, a_prob=a_prob, rows_out=rows)
        assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before


_CP = "default_env_prop.cluster_prop."
REFUSED = {      # name -> (houses, config patches) of an env the observe forms do not cover
    "state column": (20, {"default_env_prop.state_properties.hour": True}),
    "nb_agents_comm": (20, {_CP + "nb_agents_comm": 6}),
    "link defects": (20, {_CP + "comm_defect_prob": 0.2}),
    "ten houses": (10, {}),
}


def _raw_refusal(precision, env, actor, A, status):
    """The entry point through ctypes on canary-filled buffers: the documented status, a text in mdr_last_error, every byte as it was."""
    from mdr_amd import _learner as L
    from mdr_amd import _native as nat
    lib = nat.load()
    desc = L.mlp_desc(L.fc_layers(actor))
    action = torch.full((A,), 0xEE, dtype=torch.uint8, device=DEV)
    a_prob = torch.full((A,), float("nan"), device=DEV)
    probs = torch.full((A, 2), float("nan"), device=DEV)
    rows = torch.full((A, 51), float("nan"), device=DEV)
    torch.cuda.synchronize()
    spec = env._obs_spec("rows")
    rc = getattr(lib, ENTRIES[precision])(env._handle, C.byref(spec), C.byref(desc), C.c_uint64(1), C.c_uint64(2), None, 0, 0, L.ptr(action),
                                          L.ptr(a_prob), L.ptr(probs), L.ptr(rows), None)
    torch.cuda.synchronize()
    assert rc == status
    assert len(lib.mdr_last_error(env._handle).decode()) > 0
    assert bool((action == 0xEE).all()) and bool(torch.isnan(a_prob).all()) and bool(torch.isnan(probs).all()) and bool(torch.isnan(rows).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_launch_nothing(precision):
    from mdr_amd import _learner as L
    from mdr_amd import _native as nat
    from mdr_amd.sharding import LocalShardGroup
    actor = _actor()
    default = _fused(actor, precision)
    for what, (N, patches) in REFUSED.items():
        env = _fresh(2, N, patches)
        assert not default.observe_supported(env), what
        with pytest.raises(ValueError, match="sample_env"):
            default.sample_env(env, 1, 2)
        _raw_refusal(precision, env, actor, 2 * N, nat.MDR_ERR_UNSUPPORTED)
    # a house shard: half of the 24 houses of every env
    group = LocalShardGroup(_cfg(24), nb_envs=2, nb_shards=2, devices=(DEV,), seed=3)
    group.reset(episode=0)
    shard = group.shards[0]
    assert shard.sharded and shard.nb_houses == 12 and not default.observe_supported(shard)
    with pytest.raises(ValueError, match="sample_env"):
        default.sample_env(shard, 1, 2)
    _raw_refusal(precision, shard, actor, 24, nat.MDR_ERR_UNSUPPORTED)
    # an actor of another observation width on the default env
    env = _env(7, 20)
    narrow = _actor(47)
    assert not _fused(narrow, precision).observe_supported(env)
    with pytest.raises(ValueError, match="51"):
        _fused(narrow, precision).sample_env(env, 1, 2)
    _raw_refusal(precision, env, narrow, 140, nat.MDR_ERR_UNSUPPORTED)
    # ... and what mdr_mlp_actor_sample calls invalid is invalid here: a descriptor of another size, a negative grid bound
    lib = nat.load()
    desc = L.mlp_desc(L.fc_layers(actor))
    spec = env._obs_spec("rows")
    action = torch.full((140,), 0xEE, dtype=torch.uint8, device=DEV)
    fn = getattr(lib, ENTRIES[precision])
    assert fn(env._handle, C.byref(spec), C.byref(desc), C.c_uint64(1), C.c_uint64(2), None, 0, -1, L.ptr(action), None, None, None, None) == nat.MDR_ERR_INVALID
    desc.struct_size -= 8
    assert fn(env._handle, C.byref(spec), C.byref(desc), C.c_uint64(1), C.c_uint64(2), None, 0, 0, L.ptr(action), None, None, None, None) == nat.MDR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((action == 0xEE).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_collect_maddpg_transitions_with_and_without_observe_act(precision):
    from mdr_amd.rollout import collect_maddpg_transitions
    actor = _actor()
    outs, envs = [], []
    for mode in (True, False):
        env = _fresh(6, 20)
        _walk(env, 3)
        outs.append(collect_maddpg_transitions(env, actor, 3, random_steps_left=1, seed=5, actor_backend=BACKENDS[precision], observe_act=mode))
        envs.append(env)
    assert sorted(outs[0]) == sorted(outs[1]) == ["action", "reward", "state"]
    for k in outs[0]:
        assert outs[0][k].shape == outs[1][k].shape and torch.equal(outs[0][k], outs[1][k]), k
    assert bool(torch.isfinite(outs[0]["state"]).all())
    for name in ("Ta", "Tm", "sso", "flags"):
        assert torch.equal(envs[0].t[name], envs[1].t[name]), name
    assert envs[0].steps_taken == envs[1].steps_taken == 6
    assert 0.05 < outs[0]["action"][1:].float().mean().item() < 0.95      # the acting steps


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_deploy_policy_with_and_without_observe_act(precision, use_graph):
    import mdr_amd
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.rollout import deploy_policy
    E, N, T = 8, 20, 6
    actor = _actor()
    seen, results = [], []
    for mode in (True, False):
        env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device=DEV, seed=2, graph_mode=True)
        env.reset(episode=0)
        policy = GreedyDDPGActor(actor, backend=BACKENDS[precision])
        assert policy.observe_supported(env)
        seen.append(policy.sample_env(env) if mode else policy.sample(_rows(env)))
        results.append(deploy_policy(env, policy, T, seed=7, observe_act=mode, use_graph=use_graph))
        assert env.steps_taken == T
    assert torch.equal(seen[0], seen[1]) and 0 < int(seen[0].sum()) < E * N      # both actions occur
    assert bool(results[0]["reward_sum"].abs().sum() > 0)
    for name in ("reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"):
        assert torch.equal(results[0][name], results[1][name]), name
    # a FusedMLPActor passed directly draws its actions: the same through both paths
    env, twin = _fresh(E, N), _fresh(E, N)
    fused = _fused(actor, precision)
    a = deploy_policy(env, fused, 4, seed=7, observe_act=True)
    b = deploy_policy(twin, fused, 4, seed=7)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_observe_act_where_it_cannot_be_served():
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.rollout import collect_maddpg_transitions, deploy_policy
    N = 20
    actor = _actor()
    env = _fresh(2, N)
    for policy in (GreedyDDPGActor([actor] * N, backend="hip"), GreedyDDPGActor(actor, backend="torch")):
        with pytest.raises(ValueError, match="observe_act"):
            deploy_policy(env, policy, 2, observe_act=True)
    for a, backend in (([actor] * N, "hip"), (actor, "torch")):
        with pytest.raises(ValueError, match="observe_act"):
            collect_maddpg_transitions(env, a, 2, actor_backend=backend, observe_act=True)
    assert env.steps_taken == 0
    refused = _fresh(2, N, {_CP + "nb_agents_comm": 6})
    narrow = _actor(refused.obs_vector_length())
    for b in ("hip", "hip-bf16x3"):
        with pytest.raises(ValueError, match="observe_act"):
            deploy_policy(refused, GreedyDDPGActor(narrow, backend=b), 2, observe_act=True)
        with pytest.raises(ValueError, match="observe_act"):
            collect_maddpg_transitions(refused, narrow, 2, actor_backend=b, observe_act=True)
    assert refused.steps_taken == 0
