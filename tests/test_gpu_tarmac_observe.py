"""Observe -> act for the fused TarMAC actor: FusedTarMACActor.sample_env / mdr_env_tarmac_actor_sample (the observe forms of the
encode kernels in csrc/mdr_tarmac_mlp.hip and csrc/mdr_tarmac_mlp_bf16.hip) against the rows path it replaces,
fused.sample(env.obs_vector("rows"), ...).  No tolerances: the staged features are the rows' bits and the matrix instructions take
them in the same order, so every output is compared with torch.equal; the rows path itself is held to the fp64 forward by
tests/test_gpu_tarmac_fused.py and tests/test_gpu_tarmac_bf16.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = ["fp32", "bf16x3"]
# (3, 11): the smallest env, its window wraps onto the whole env, A = 33 ends in a partial tile; (7, 20): tiles that span envs;
# (4, 32): the aligned staging path in both precisions; (2, 300): slices and halos in the attention
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


def _env(E, N, **patches):
    """An env a dozen random steps into its episode - lockouts, seconds_since_off and on / off flags mixed - built once per shape
    and never stepped again: sampling does not change it."""
    import mdr_amd
    key = (E, N, tuple(sorted(patches.items())))
    if key not in _ENVS:
        env = mdr_amd.BatchedDemandResponseEnv(_cfg(N, **patches), nb_envs=E, device=DEV, seed=5 + N)
        env.reset(episode=0)
        _walk(env, 12, seed=N)
        _ENVS[key] = env
    return _ENVS[key]


def _actor(F=51, H=64, K=8, V=16, c=10, hops=1, seed=11, **kw):
    from mdr_amd.tarmac import TarMACActor
    torch.manual_seed(seed)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=c, num_hops=hops, **kw)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return actor.to(DEV)


def _fused(actor, precision):
    from mdr_amd.tarmac import FusedTarMACActor
    return FusedTarMACActor.from_module(actor, precision)


def _both(fused, env, seed=9, step=4, **kw):
    by_rows = fused.sample(env.obs_vector("rows"), seed, step, want_probs=True, **kw)
    by_state = fused.sample_env(env, seed, step, want_probs=True, **kw)
    return by_rows, by_state


def _assert_equal(by_rows, by_state, what):
    for name, a, b in zip(("action", "a_prob", "probs"), by_rows, by_state):
        assert a.shape == b.shape and torch.equal(a, b), "%s: %s differs from the rows path" % (what, name)
    assert bool(torch.isfinite(by_state[2]).all()), what


VARIANTS = {
    "one_hop": (dict(), dict()),
    "two_hops": (dict(hops=2), dict()),
    "no_comm": (dict(with_comm=False), dict()),
    "attention_defects": (dict(comm_defect_prob=0.3), dict()),
    "greedy": (dict(), dict(greedy=True)),
    "step_dev": (dict(hops=2), dict(step_dev=True)),
    "general_form": (dict(H=32, K=4, V=8, hops=2), dict()),      # not the reference's sizes: the run-time block counts
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sample_env_equals_sample_on_the_rows(precision, variant):
    actor_kw, call_kw = VARIANTS[variant]
    fused = _fused(_actor(**actor_kw), precision)
    call_kw = dict(call_kw)
    if call_kw.pop("step_dev", False):
        call_kw["step_dev"] = torch.tensor([5], dtype=torch.int32, device=DEV)
    for E, N in SHAPES:
        env = _env(E, N)
        assert fused.observe_supported(env)
        by_rows, by_state = _both(fused, env, **call_kw)
        _assert_equal(by_rows, by_state, "%s %s E%d N%d" % (precision, variant, E, N))
    spread = by_state[2][:, 0]
    assert 0.02 < float(spread.mean()) < 0.98 and float(spread.std()) > 0.01      # not a saturated actor


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_stride_restages_the_window(precision):
    """(1400, 50): 4375 tiles of 16 (2188 of 32), more than the persistent grid has waves (256 CUs x 16 | 8): every wave stages its
    window again and again, loading the next tile under the current one's matrix work."""
    env = _env(1400, 50)
    fused = _fused(_actor(hops=2), precision)
    by_rows, by_state = _both(fused, env)
    _assert_equal(by_rows, by_state, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rows_out_is_obs_vector_rows(precision):
    fused = _fused(_actor(), precision)
    for E, N in SHAPES + [(1400, 50)]:
        env = _env(E, N)
        A = E * N
        rows = env.obs_vector("rows").view(A, 51)
        plain = fused.sample_env(env, 9, 4, want_probs=True)
        wide = torch.full((A + 2, 51), -7.0, device=DEV)      # a row of sentinels before and behind the rows
        kept = fused.sample_env(env, 9, 4, want_probs=True, rows_out=wide[1:A + 1])
        assert torch.equal(wide[1:A + 1], rows), "rows_out differs from obs_vector('rows') at E%d N%d" % (E, N)
        assert bool((wide[0] == -7.0).all()) and bool((wide[A + 1] == -7.0).all())
        _assert_equal(plain, kept, "with rows_out E%d N%d" % (E, N))
    # a per-step slice of a transition buffer that is not 16-byte aligned (A * 51 odd): the 4-byte store path
    env = _env(3, 11)
    buf = torch.full((2, 33, 51), -7.0, device=DEV)
    fused.sample_env(env, 9, 4, rows_out=buf[1])
    assert torch.equal(buf[1], env.obs_vector("rows").view(33, 51)) and bool((buf[0] == -7.0).all())


def _fresh(E, N, patches, **kw):
    import mdr_amd
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N, **patches), nb_envs=E, device=DEV, seed=4, **kw)
    env.reset(episode=0)
    return env


_CP = "default_env_prop.cluster_prop."
REFUSED = {      # name -> (houses, config patches) of an env the observe forms do not cover
    "state column": (20, {"default_env_prop.state_properties.hour": True}),
    "nb_agents_comm": (20, {_CP + "nb_agents_comm": 6}),
    "link defects": (20, {_CP + "comm_defect_prob": 0.2}),
    "ten houses": (10, {}),
}


def _raw_refusal(lib, env, fused, A):
    """mdr_env_tarmac_actor_sample through ctypes on sentinel-filled buffers: MDR_ERR_UNSUPPORTED and every byte as it was."""
    from mdr_amd import _native as nat
    st = fused._pack()
    action = torch.full((A,), 77, dtype=torch.uint8, device=DEV)
    a_prob = torch.full((A,), -7.0, device=DEV)
    probs = torch.full((A, 2), -7.0, device=DEV)
    rows = torch.full((A, 51), -7.0, device=DEV)
    ws = fused.workspace(A, torch.device(DEV))
    ws.fill_(0x5A)
    torch.cuda.synchronize()
    spec = env._obs_spec("rows")
    rc = lib.mdr_env_tarmac_actor_sample(env._handle, C.byref(spec), C.byref(st), C.c_uint64(1), C.c_uint64(2), None, C.c_void_p(ws.data_ptr()),
                                         C.c_void_p(action.data_ptr()), C.c_void_p(a_prob.data_ptr()), C.c_void_p(probs.data_ptr()),
                                         C.c_void_p(rows.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == nat.MDR_ERR_UNSUPPORTED
    assert bool((action == 77).all()) and bool((a_prob == -7.0).all()) and bool((probs == -7.0).all()) and bool((rows == -7.0).all())
    assert bool((ws == 0x5A).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_launch_nothing(precision):
    from mdr_amd import _native as nat
    from mdr_amd.rollout import collect_tarmac_rollout, deploy_policy
    from mdr_amd.sharding import LocalShardGroup
    lib = nat.load()
    default = _fused(_actor(), precision)
    for what, (N, patches) in REFUSED.items():
        env = _fresh(2, N, patches)
        F = env.obs_vector_length()
        fused = default if F == 51 else _fused(_actor(F), precision)      # the actor this env's rows need
        assert not fused.observe_supported(env), what
        with pytest.raises(ValueError):
            fused.sample_env(env, 1, 2)
        _raw_refusal(lib, env, default, 2 * N)
        with pytest.raises(ValueError):
            collect_tarmac_rollout(env, fused, 2, observe_act=True)
        with pytest.raises(ValueError):
            deploy_policy(env, fused, 2, observe_act=True)
        assert env.steps_taken == 0
        ro = collect_tarmac_rollout(env, fused, 2, seed=3)      # observe_act=None: through the rows
        twin = _fresh(2, N, patches)
        assert torch.equal(ro["state"][0], twin.obs_vector("rows").view(2 * N, F))
        a, ap = fused.sample(twin.obs_vector("rows"), 3, 0)
        assert torch.equal(ro["action"][0], a.to(torch.int64)) and torch.equal(ro["a_prob"][0], ap)
    # a house shard: half of the 24 houses of every env
    group = LocalShardGroup(_cfg(24), nb_envs=2, nb_shards=2, devices=(DEV,), seed=3)
    group.reset(episode=0)
    shard = group.shards[0]
    assert shard.sharded and shard.nb_houses == 12 and not default.observe_supported(shard)
    with pytest.raises(ValueError):
        default.sample_env(shard, 1, 2)
    _raw_refusal(lib, shard, default, 24)
    # an actor of another observation width on the default env
    env = _env(2, 20)
    narrow = _fused(_actor(47), precision)
    assert not narrow.observe_supported(env)
    with pytest.raises(ValueError):
        narrow.sample_env(env, 1, 2)
    _raw_refusal(lib, env, narrow, 40)
    # ... and a TarMACActor that is not fused cannot be asked for it
    with pytest.raises(ValueError):
        collect_tarmac_rollout(_fresh(2, 20, {}), _actor(), 2, observe_act=True)


def test_sample_env_allocates_nothing_after_the_first_call():
    env = _env(5, 50)
    fused = _fused(_actor(hops=2), "fp32")
    A = 250
    action = torch.empty(A, dtype=torch.uint8, device=DEV)
    a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
    rows = torch.empty((A, 51), device=DEV)
    fused.sample_env(env, 1, 0, action=action, a_prob=a_prob, rows_out=rows)
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    for t in range(3):
        fused.sample_env(env, 1, t, action=action, a_prob=a_prob, rows_out=rows)
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before


@pytest.mark.parametrize("store_states", [True, False])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_collect_tarmac_rollout_with_and_without_observe_act(precision, store_states):
    from mdr_amd.rollout import collect_tarmac_rollout
    from mdr_amd.tarmac import TarMACCritic
    E, N, T = 6, 20, 5
    fused = _fused(_actor(hops=2), precision)
    torch.manual_seed(2)
    critic = TarMACCritic(N, 51).to(DEV)
    outs, envs = [], []
    for mode in (True, False, None):
        env = _fresh(E, N, {})
        _walk(env, 3)
        outs.append(collect_tarmac_rollout(env, fused, T, gamma=0.9, critic=critic, seed=5, store_states=store_states, observe_act=mode))
        envs.append(env)
    assert ("state" in outs[0]) == store_states
    for other in outs[1:]:
        assert sorted(other) == sorted(outs[0])
        for k in outs[0]:
            assert torch.equal(outs[0][k], other[k]), k
    for name in ("Ta", "Tm", "sso", "flags", "obs"):
        assert torch.equal(envs[0].t[name], envs[1].t[name]), name
    assert envs[0]._obs_planes_on and envs[0].steps_taken == envs[1].steps_taken == 3 + T
    assert 0.05 < outs[0]["action"].float().mean().item() < 0.95


@pytest.mark.parametrize("precision", PRECISIONS)
def test_deploy_policy_with_and_without_observe_act(precision):
    """Eager and captured (table_steps = 16 and 40 steps: the replays cross two table refills), greedy or drawn."""
    import mdr_amd
    from mdr_amd.rollout import deploy_policy
    E, N, T = 4, 20, 40
    fused = _fused(_actor(hops=2, comm_defect_prob=0.2), precision)
    results = {}
    for use_graph in (False, True):
        for mode in (True, False, None):
            env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device=DEV, seed=2, table_steps=16, graph_mode=True)
            env.reset(episode=0)
            results[(use_graph, mode)] = deploy_policy(env, fused, T, seed=7, use_graph=use_graph, observe_act=mode)
    first = results[(False, False)]
    assert bool(first["reward_sum"].abs().sum() > 0)
    for key, other in results.items():
        for name in ("reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"):
            assert torch.equal(first[name], other[name]), (key, name)
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device=DEV, seed=2)
    env.reset(episode=0)
    twin = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device=DEV, seed=2)
    twin.reset(episode=0)
    a = deploy_policy(env, fused, 6, seed=7, greedy=True, observe_act=True)
    b = deploy_policy(twin, fused, 6, seed=7, greedy=True, observe_act=False)
    for name in a:
        assert torch.equal(a[name], b[name]), name
