"""mdr_env_bind_hvac_code: the single-step kernels read a house's (Q_hvac, P_max) pair through one class byte and a 16-entry
dictionary instead of streaming the two columns.  Held bit for bit to the same env without the code (hvac_code=False) in every
kernel form behind the two shared loaders; the detection kernel against the rule (distinct raw-bit pairs, at most 16) and against
the three buffers read back: dict[class[i]] is (Q_hvac[i], P_max[i]) at every house."""
import copy

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat

pytestmark = pytest.mark.gpu

OUT = ("Ta", "Tm", "sso", "flags", "reward", "obs", "P", "actions")
STEPS = 70      # table_steps = 64: the run crosses one refill

# (E, N, sharded through a mailbox step): the shapes of tests/test_gpu_uniform_params.py - every kernel form behind the loaders
SHAPES = {
    "fused_1024": (3, 1024, False),      # k_step_fused<4,1,256>
    "fused_2048": (2, 2048, False),      # two tiles
    "vec1_300": (4, 300, False),         # one house per lane, last wave partly filled
    "group_50": (40, 50, False),         # several envs per workgroup
    "split_5000": (3, 5000, False),      # partial + finish kernels
    "mailbox_6100": (1, 6100, True),     # k_step_mailbox: a world of one on one device
}
# noise_hvac_prop.noise_mode -> distinct (Q_hvac, P_max) pairs: the length of its cooling_capacity_list (one COP, one latent fraction)
COUNTS = {"big_noise": 5, "small_noise": 3, "no_noise": 1}


def _cfg(n, hvac_noise="big_noise"):
    import mdr_amd
    cfg = mdr_amd.default_config()
    env = cfg["default_env_prop"]
    env["cluster_prop"]["nb_agents"] = n
    env["cluster_prop"]["temp_mode"] = "noisy_sinusoidal_heatwave"
    env["power_grid_prop"]["base_power_mode"] = "constant"
    env["power_grid_prop"]["signal_mode"] = "perlin"
    env["start_datetime_mode"] = "random"
    cfg["noise_house_prop"]["noise_mode"] = "house_big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = hvac_noise
    cfg["default_hvac_prop"]["lockout_noise"] = 0
    cfg["default_house_prop"]["solar_gain_bool"] = True
    return cfg


def _env(cfg, E, N, sharded, coded, seed=77):
    import mdr_amd
    kw = {}
    if sharded:
        from mdr_amd.sharding import MailboxExchange
        kw = dict(house_shard=(0, N), exchange_always=True, exchange=MailboxExchange())
    return mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=64, hvac_code=coded, **kw)


def _count(env):
    return int(env.t["hvac_dict"][nat.MDR_HVAC_DICT_COUNT].item())


def _word(env):
    return int(env.t["param_uniform"].item())


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _rule(env):
    """Distinct raw-bit pairs of the env's two arrays (tests/test_hvac_code.py restates the rule in full)."""
    keys = (_bits(env.t["P_max"]).astype(np.uint64) << np.uint64(32)) | _bits(env.t["Q_hvac"]).astype(np.uint64)
    return len(np.unique(keys))


def _check_code(env, count):
    """The count, and on the host from the three buffers: dict[class[i]] == (Q_hvac[i], P_max[i]) bit for bit at every house."""
    assert _count(env) == count == _rule(env)
    d = env.t["hvac_dict"].cpu().numpy().view(np.uint32)
    cls = env.t["hvac_class"].cpu().numpy().astype(np.int64)
    assert cls.shape == (env.nb_envs, env.nb_houses) and int(cls.max()) < count
    assert np.array_equal(d[2 * cls], _bits(env.t["Q_hvac"]))
    assert np.array_equal(d[2 * cls + 1], _bits(env.t["P_max"]))
    assert len(np.unique(cls)) == count      # every entry is some house's


def _same(a, b, where):
    for name in OUT:
        assert torch.equal(a.t[name], b.t[name]), (where, name)


def _step_both(envs, kind, gen):
    if kind == "bangbang":
        for env in envs:
            env.step_bangbang()
    else:
        first = envs[0]
        act = (torch.rand((first.nb_envs, first.nb_houses), generator=gen, device="cuda:0") < 0.6).to(torch.uint8)
        for env in envs:
            env.step(act)
            env.t["actions"].copy_(act)      # an external step leaves the caller's plane alone: keep `actions` comparable


def _run_twins(envs, steps, gen, where):
    for t in range(steps):
        _step_both(envs, "bangbang" if t % 2 else "external", gen)
        for other in envs[1:]:
            _same(envs[0], other, (where, t))


# ------------------------------------------------------------------------------------------------ 1. twin runs
@pytest.mark.parametrize("kind", ["external", "bangbang"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_twin_runs_are_bit_identical(shape, kind):
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N)
    coded = _env(cfg, E, N, sharded, True)
    plain = _env(cfg, E, N, sharded, False)
    coded.reset(episode=1)
    plain.reset(episode=1)
    _check_code(coded, COUNTS["big_noise"])
    assert "hvac_dict" not in plain.t and "hvac_class" not in plain.t
    assert _word(coded) == _word(plain) == 7      # param_uniform is what it was
    gen = torch.Generator(device="cuda:0").manual_seed(1000 + N)
    for t in range(STEPS):
        _step_both((coded, plain), kind, gen)
        _same(coded, plain, t)
    assert coded.steps_taken == STEPS
    _check_code(coded, COUNTS["big_noise"])
    assert _word(coded) == 7


@pytest.mark.parametrize("noise", ["small_noise", "no_noise"])
@pytest.mark.parametrize("shape", ["fused_1024", "group_50"])
def test_count_follows_the_capacity_list(shape, noise):
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N, noise)
    coded = _env(cfg, E, N, sharded, True)
    plain = _env(cfg, E, N, sharded, False)
    coded.reset(episode=1)
    plain.reset(episode=1)
    _check_code(coded, COUNTS[noise])
    _run_twins((coded, plain), 6, torch.Generator(device="cuda:0").manual_seed(2), noise)


# ------------------------------------------------------------------------------------------------ 2. the coded columns are not read
@pytest.mark.parametrize("shape", ["fused_1024", "fused_2048", "group_50"])
def test_coded_columns_are_not_read(shape):
    """With a count > 0 the two arrays can hold anything: the step never sees it."""
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N)
    coded = _env(cfg, E, N, sharded, True)
    plain = _env(cfg, E, N, sharded, False)
    coded.reset(episode=3)
    plain.reset(episode=3)
    assert _count(coded) == 5
    coded.t["Q_hvac"].fill_(float("nan"))
    coded.t["P_max"].fill_(float("nan"))      # (no params_changed(): the dictionary still holds the pairs)
    _run_twins((coded, plain), 10, torch.Generator(device="cuda:0").manual_seed(5), "nan")
    assert torch.isfinite(coded.t["reward"]).all() and torch.isfinite(coded.t["obs"]).all()


# ------------------------------------------------------------------------------------------------ 3. detection
def _write_pairs(envs, q, p):
    for env in envs:
        env.t["Q_hvac"].copy_(torch.from_numpy(q).to("cuda:0"))
        env.t["P_max"].copy_(torch.from_numpy(p).to("cuda:0"))
        env.params_changed()


def _sixteen(E, N, seed):
    """16 distinct pairs spread over [E, N]; every one of them occurs (the first 16 houses hold one each)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 16, size=E * N)
    idx[:16] = np.arange(16)
    qv = -(6000.0 + 500.0 * np.arange(16)).astype(np.float32)
    pv = (2000.0 + 250.0 * np.arange(16)).astype(np.float32)
    return qv[idx].reshape(E, N).copy(), pv[idx].reshape(E, N).copy()


@pytest.mark.parametrize("E,N", [(3, 301), (2, 2048)])      # 903 elements: a scalar tail behind the 16-byte body; 4096: none
def test_detection_sixteen_pairs_and_a_seventeenth_anywhere(E, N):
    cfg = _cfg(N)
    coded = _env(cfg, E, N, False, True)
    plain = _env(cfg, E, N, False, False)
    coded.reset(episode=0)
    plain.reset(episode=0)
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    q, p = _sixteen(E, N, N)
    _write_pairs((coded, plain), q, p)
    _check_code(coded, 16)
    _run_twins((coded, plain), 4, gen, "sixteen")
    n = E * N
    for pos in (1, n // 2, n - 1):
        q17, p17 = q.copy(), p.copy()
        q17.reshape(-1)[pos] = -12345.0      # a 17th pair: the count says "not coded" and everything streams
        _write_pairs((coded, plain), q17, p17)
        assert _count(coded) == 0 and _rule(coded) == 17, pos
        _run_twins((coded, plain), 3, gen, ("seventeen", pos))
        _write_pairs((coded, plain), q, p)
        _check_code(coded, 16)
    _run_twins((coded, plain), 3, gen, "sixteen again")


@pytest.mark.parametrize("E,N", [(3, 301), (2, 2048)])
def test_detection_compares_both_words_bitwise(E, N):
    cfg = _cfg(N)
    coded = _env(cfg, E, N, False, True)
    plain = _env(cfg, E, N, False, False)
    coded.reset(episode=0)
    plain.reset(episode=0)
    gen = torch.Generator(device="cuda:0").manual_seed(12)
    n = E * N
    # equal Q_hvac, different P_max: two entries
    q = np.full((E, N), -9000.0, dtype=np.float32)
    p = np.full((E, N), 3000.0, dtype=np.float32)
    p.reshape(-1)[n - 1] = 3500.0
    _write_pairs((coded, plain), q, p)
    _check_code(coded, 2)
    _run_twins((coded, plain), 3, gen, "P_max differs")
    # ... and the other way round
    q.reshape(-1)[n // 2] = -9500.0
    p.reshape(-1)[n // 2] = 3000.0
    _write_pairs((coded, plain), q, p)
    _check_code(coded, 3)
    # -0.0 against +0.0 in P_max: two entries
    p = np.zeros((E, N), dtype=np.float32)
    p.reshape(-1)[1::2] = -0.0
    q = np.full((E, N), -9000.0, dtype=np.float32)
    _write_pairs((coded, plain), q, p)
    _check_code(coded, 2)
    _run_twins((coded, plain), 3, gen, "signed zero")
    # NaN payloads count, and the all-ones pair - the kernel's mark of a free slot - cannot be coded
    p = np.full((E, N), 3000.0, dtype=np.float32)
    p.view(np.uint32).reshape(-1)[0] = 0x7FC00001
    p.view(np.uint32).reshape(-1)[n - 1] = 0x7FC00002
    _write_pairs((coded,), q, p)
    _check_code(coded, 3)
    q.view(np.uint32).reshape(-1)[n - 1] = 0xFFFFFFFF
    p.view(np.uint32).reshape(-1)[n - 1] = 0xFFFFFFFF
    _write_pairs((coded,), q, p)
    assert _count(coded) == 0


def _raw_params(env):
    """What load_episode takes (fp64, deg C), read back from a reset env."""
    t, ref = env.t, env.spec.temp_ref
    p = {name: t[name].double().cpu().numpy() for name in ("deadband", "Ua", "Cm", "Ca", "Hm", "capacity", "COP", "latent")}
    for name in ("Ta", "Tm", "target"):
        p[name] = t[name].double().cpu().numpy() + ref
    p["lockout"] = t["lockout"].cpu().numpy().astype(np.int64)
    p["t0"] = t["t0"].cpu().numpy()
    p["phase"] = t["phase"].cpu().numpy()
    p["ratio"] = t["ratio"].cpu().numpy()
    return p


@pytest.mark.parametrize("E,N", [(3, 301), (2, 2048)])
def test_load_episode_with_per_house_cop(E, N):
    """Per-house COP (the reference's commented-out noise, reachable through load_episode): equal Q_hvac under different P_max."""
    cfg = _cfg(N)
    src = _env(cfg, E, N, False, True)
    src.reset(episode=2)
    raw = _raw_params(src)
    raw["COP"] = raw["COP"] * np.where(np.random.default_rng(N).random((E, N)) < 0.5, 1.0, 1.25)
    coded = _env(cfg, E, N, False, True)
    plain = _env(cfg, E, N, False, False)
    coded.load_episode(raw, seed=77, episode=2)
    plain.load_episode(raw, seed=77, episode=2)
    assert len(np.unique(_bits(coded.t["Q_hvac"]))) == 5
    _check_code(coded, 10)
    _run_twins((coded, plain), 6, torch.Generator(device="cuda:0").manual_seed(13), "per-house COP")


# ------------------------------------------------------------------------------------------------ 4. snapshots
def test_snapshots_continue_bit_identically():
    """copy.deepcopy and state_dict -> load_state_dict into a fresh env, with the code on both sides and on one side only: the
    snapshot is the slab as it always was, the code is rebuilt from its arrays."""
    E, N, sharded = SHAPES["fused_1024"]
    cfg = _cfg(N)
    coded = _env(cfg, E, N, sharded, True)
    plain = _env(cfg, E, N, sharded, False)
    coded.reset(episode=4)
    plain.reset(episode=4)
    for _ in range(5):
        coded.step_bangbang()
        plain.step_bangbang()
    twin = copy.deepcopy(coded)
    assert "hvac_dict" in twin.t and "hvac_dict" not in copy.deepcopy(plain).t      # the flag travels
    coded2coded, coded2plain, plain2coded = _env(cfg, E, N, sharded, True), _env(cfg, E, N, sharded, False), _env(cfg, E, N, sharded, True)
    sd = coded.state_dict()
    assert sd["slab"].numel() == plain.state_dict()["slab"].numel()      # one layout: a snapshot from before the code loads as well
    coded2coded.load_state_dict(sd)
    coded2plain.load_state_dict(sd)
    plain2coded.load_state_dict(plain.state_dict())
    for env in (twin, coded2coded, plain2coded):
        _check_code(env, 5)
    _run_twins((coded, plain, twin, coded2coded, coded2plain, plain2coded), 10, torch.Generator(device="cuda:0").manual_seed(8), "snapshots")
