"""mdr_buffers_t.param_uniform: the step kernels take the per-house columns that hold one value for every house (target, deadband,
lockout - bits 0, 1, 2 of a device word written at reset / load_episode / params_changed) from element [0] instead of streaming
them.  Held bit for bit to the same env with the word unbound (uniform_params=False: every column streamed), in every
single-step kernel form: the reference samples these three per house (utils.py:623-676, env/MA_DemandResponse.py:430) and the
step reads them per house (env 478-492, 263-326), so a skipped column may never change a result."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OUT = ("Ta", "Tm", "sso", "flags", "reward", "obs", "P", "actions")
STEPS = 70      # table_steps = 64: the run crosses one refill

# (E, N, sharded through a mailbox step)
SHAPES = {
    "fused_1024": (3, 1024, False),      # k_step_fused<4,1,256>
    "fused_2048": (2, 2048, False),      # two tiles
    "vec1_300": (4, 300, False),         # one house per lane
    "group_50": (40, 50, False),         # several envs per workgroup
    "split_5000": (3, 5000, False),      # partial + finish kernels
    "mailbox_6100": (1, 6100, True),     # k_step_mailbox: a world of one on one device
}
# configuration -> the word it must produce
CONFIGS = {"c3": 7, "lockout_noise": 3, "big_noise": 6, "deadband": 7}


def _cfg(n, variant):
    import mdr_amd
    cfg = mdr_amd.default_config()
    env = cfg["default_env_prop"]
    env["cluster_prop"]["nb_agents"] = n
    env["cluster_prop"]["temp_mode"] = "noisy_sinusoidal_heatwave"
    env["power_grid_prop"]["base_power_mode"] = "constant"
    env["power_grid_prop"]["signal_mode"] = "perlin"
    env["start_datetime_mode"] = "random"
    cfg["noise_house_prop"]["noise_mode"] = "house_big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    cfg["default_hvac_prop"]["lockout_noise"] = 0
    cfg["default_house_prop"]["solar_gain_bool"] = True
    if variant == "lockout_noise":
        cfg["default_hvac_prop"]["lockout_noise"] = 10
    elif variant == "big_noise":
        cfg["noise_house_prop"]["noise_mode"] = "big_noise"      # std_target_temp 2
    elif variant == "deadband":
        cfg["default_house_prop"]["deadband"] = 0.5
    else:
        assert variant == "c3"
    return cfg


def _env(cfg, E, N, sharded, uniform, seed=77):
    import mdr_amd
    kw = {}
    if sharded:
        from mdr_amd.sharding import MailboxExchange
        kw = dict(house_shard=(0, N), exchange_always=True, exchange=MailboxExchange())
    return mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=64, uniform_params=uniform, **kw)


def _word(env):
    return int(env.t["param_uniform"].item())


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


@pytest.mark.parametrize("kind", ["external", "bangbang"])
@pytest.mark.parametrize("variant", list(CONFIGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_twin_runs_are_bit_identical(shape, variant, kind):
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N, variant)
    uni = _env(cfg, E, N, sharded, True)
    ref = _env(cfg, E, N, sharded, False)
    uni.reset(episode=1)
    ref.reset(episode=1)
    assert _word(uni) == CONFIGS[variant]
    assert _word(ref) == 0      # not bound: never written
    gen = torch.Generator(device="cuda:0").manual_seed(1000 + N)
    for t in range(STEPS):
        _step_both((uni, ref), kind, gen)
        _same(uni, ref, t)
    assert uni.steps_taken == STEPS
    assert _word(uni) == CONFIGS[variant]


@pytest.mark.parametrize("shape", ["fused_1024", "fused_2048", "group_50"])
def test_uniform_columns_are_not_read(shape):
    """With word 7 the three arrays behind element [0] can hold anything: the step never sees it."""
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N, "c3")
    uni = _env(cfg, E, N, sharded, True)
    ref = _env(cfg, E, N, sharded, False)
    uni.reset(episode=3)
    ref.reset(episode=3)
    assert _word(uni) == 7
    uni.t["target"][..., 1:] = float("nan")
    uni.t["deadband"][..., 1:] = float("nan")
    uni.t["lockout"][..., 1:] = -1      # (no params_changed(): the word still says uniform)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    for t in range(10):
        _step_both((uni, ref), "bangbang" if t % 2 else "external", gen)
        for name in OUT:
            assert torch.equal(uni.t[name], ref.t[name]), (t, name)
    assert torch.isfinite(uni.t["reward"]).all() and torch.isfinite(uni.t["obs"]).all()


@pytest.mark.parametrize("E,N", [(3, 301), (2, 2048)])      # 903 elements: a scalar tail behind the 16-byte body; 4096: none
def test_detection_sees_one_differing_element_anywhere(E, N):
    """params_changed() compares bitwise with element [0]: one differing element - the second, a middle one, the very last -
    clears exactly its column's bit; -0.0 is not +0.0."""
    env = _env(_cfg(N, "c3"), E, N, False, True)
    env.reset(episode=0)
    assert _word(env) == 7
    n = E * N
    for bit, name in enumerate(("target", "deadband", "lockout")):
        flat = env.t[name].view(-1)
        for pos in (1, n // 2, n - 1, 0):      # (element [0] itself: every other element then differs)
            keep = flat[pos].clone()
            flat[pos] = flat[pos] + 1
            env.params_changed()
            assert _word(env) == 7 & ~(1 << bit), (name, pos)
            flat[pos] = keep
            env.params_changed()
            assert _word(env) == 7, (name, pos)
    assert float(env.t["deadband"].view(-1)[0]) == 0.0
    env.t["deadband"].view(-1)[n - 2] = -0.0
    env.params_changed()
    assert _word(env) == 5


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


@pytest.mark.parametrize("shape", ["fused_1024", "split_5000"])
def test_params_changed_invalidates_and_matches_load_episode(shape):
    E, N, sharded = SHAPES[shape]
    cfg = _cfg(N, "c3")
    src = _env(cfg, E, N, sharded, True)
    src.reset(episode=2)
    base = _raw_params(src)
    moved = dict(base)
    moved["target"] = base["target"] + np.random.default_rng(9).integers(0, 5, size=(E, N)) * 0.25      # exact in fp32
    a = _env(cfg, E, N, sharded, True)
    b = _env(cfg, E, N, sharded, True)
    a.load_episode(base, seed=77, episode=2)
    b.load_episode(moved, seed=77, episode=2)
    assert _word(a) == 7 and _word(b) == 6
    a.t["target"].copy_(b.t["target"])
    a.params_changed()
    assert _word(a) == 6
    for name in ("target", "deadband", "lockout", "Ta", "Tm", "k01", "s0", "k10", "s1", "inv_Ua", "Q_hvac", "P_max"):
        assert torch.equal(a.t[name], b.t[name]), name
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for t in range(12):
        _step_both((a, b), "bangbang" if t % 2 else "external", gen)
        _same(a, b, t)


@pytest.mark.parametrize("variant", ["c3", "big_noise"])
def test_snapshots_continue_bit_identically(variant):
    """copy.deepcopy and a state_dict / load_state_dict round trip carry the word with the arrays."""
    E, N, sharded = SHAPES["fused_1024"]
    cfg = _cfg(N, variant)
    env = _env(cfg, E, N, sharded, True)
    env.reset(episode=4)
    for _ in range(5):
        env.step_bangbang()
    twin = copy.deepcopy(env)
    other = _env(cfg, E, N, sharded, True)
    other.t["param_uniform"].fill_(7 ^ CONFIGS[variant])      # whatever it held: load_state_dict derives it again
    other.load_state_dict(env.state_dict())
    assert _word(env) == _word(twin) == _word(other) == CONFIGS[variant]
    gen = torch.Generator(device="cuda:0").manual_seed(8)
    for t in range(10):
        _step_both((env, twin, other), "bangbang" if t % 2 else "external", gen)
        _same(env, twin, ("deepcopy", t))
        _same(env, other, ("state_dict", t))
