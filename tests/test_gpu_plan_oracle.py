"""Every step and rollout form the planner can launch (tests/plan_util.py: reachable_forms) against the fp64 oracle, at the smallest
batch that selects it - device-filling batches included, where the small-batch suites never go - and a seeded fuzz of
device-filling batches of small envs.  The oracle runs on a few envs of the full device batch (tests/slice_oracle.py)."""
import math

import numpy as np
import pytest
import torch

from tests import plan_util as pu
from tests.slice_oracle import SliceOracle

pytestmark = pytest.mark.gpu

CASES = pu.oracle_cases()
STEP_CASES = [(i, c) for i, c in enumerate(CASES) if c[3] is None]
ROLLOUT_CASES = [(i, c) for i, c in enumerate(CASES) if c[3] is not None]
PENALTIES = ("individual_L2", "common_L2", "common_max", "mixture")
SIGNALS = ("perlin", "sinusoidals")
TABLE_STEPS, T = 32, 70       # two table refills (steps 32 and 64) inside the run


def _id(ic):
    i, (form, N, E, ctl) = ic
    return "%s-N%d-E%d" % (form, N, E)


def _cfg(N, i):
    import mdr_amd
    cfg = mdr_amd.default_config()
    env = cfg["default_env_prop"]
    env["cluster_prop"]["nb_agents"] = N
    env["cluster_prop"]["temp_mode"] = "noisy_sinusoidal_heatwave"
    env["start_datetime_mode"] = "random"
    pg = env["power_grid_prop"]
    pg["base_power_mode"] = "constant"
    pg["signal_mode"] = SIGNALS[(i // 4) % 2]
    pg["artificial_signal_ratio_range"] = 2
    rw = env["reward_prop"]
    rw["temp_penalty_mode"] = PENALTIES[i % 4]
    rw["temp_penalty_parameters"]["mixture"] = {"alpha_ind_L2": 0.7, "alpha_common_L2": 1.3, "alpha_common_max": 0.4}
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    cfg["default_hvac_prop"]["lockout_noise"] = 12
    cfg["default_house_prop"]["deadband"] = 0.5
    cfg["default_house_prop"]["solar_gain_bool"] = True
    return cfg


def _env(cfg, E, seed, table_steps=TABLE_STEPS):
    import mdr_amd
    return mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=table_steps)


@pytest.mark.parametrize("ic", STEP_CASES, ids=_id)
def test_step_form_vs_oracle(ic):
    """T single steps of random external actions and in-kernel bang-bang (every third step, replayed in the oracle; its decisions
    against the oracle's rule), every step on the first / middle / last envs against the oracle."""
    i, (form, N, E, _) = ic
    assert pu.step_kernel(N, E) == form
    cfg = _cfg(N, i)
    seed, episode = 7919 * i + 13, i % 3
    env = _env(cfg, E, seed)
    env.reset(episode=episode)
    sl = SliceOracle(cfg, env, seed, episode)
    sl.check(env, "%s after reset" % form, reward=False, obs=False)
    gen = torch.Generator(device="cuda:0").manual_seed(i)
    for t in range(T):
        where = "%s (N=%d E=%d) step %d" % (form, N, E, t)
        if t % 3 == 2:
            want = sl.decisions("bangbang")
            env.step_bangbang()
            acts = sl.take(env.t["actions"])
            diff, off_edge = sl.decision_misses(acts, "bangbang", want)
            assert off_edge == 0, "%s: %d bang-bang decisions differ away from the threshold" % (where, off_edge)
        else:
            act = (torch.rand((E, N), device="cuda:0", generator=gen) < 0.55).to(torch.uint8)
            env.step(act)
            acts = sl.take(act)
        sl.step(acts)
        sl.check(env, where)


def _controller_run(a, sl, kind, where):
    """One controller step on `a` (single-step path), its decisions against the oracle's rule, the oracle replaying them."""
    want = sl.decisions(kind)
    _, r, _, _ = a.step_controller()
    acts = sl.take(a.t["actions"])
    diff, off_edge = sl.decision_misses(acts, kind, want)
    assert off_edge == 0, "%s: %d %s decisions differ away from a threshold" % (where, off_edge, kind)
    sl.step(acts)
    sl.check(a, where)
    return r


@pytest.mark.parametrize("ic", ROLLOUT_CASES, ids=_id)
def test_rollout_form_vs_single_steps_vs_oracle(ic):
    """rollout_fused(T) equals T single controller steps bit for bit (state, reward, obs planes, actions, power trace, reward sum),
    and those steps match the oracle on three slices.  For the forms of the other controllers (BB = false) also always_on and
    deadband through rollout_fused directly against the oracle's own rule, in chunks that cross the table refills."""
    i, (form, N, E, ctl) = ic
    assert pu.rollout_kernel(N, E, ctl) == form
    cfg = _cfg(N, i)
    seed, episode = 7919 * i + 29, i % 3
    a, b = _env(cfg, E, seed), _env(cfg, E, seed)
    for env in (a, b):
        env.reset(episode=episode)
        env.set_controller(ctl)
    sl = SliceOracle(cfg, a, seed, episode)
    rsum = torch.zeros((E, N), dtype=torch.float32, device="cuda:0")
    trace = []
    for t in range(T):
        rsum += _controller_run(a, sl, ctl, "%s (N=%d E=%d) step %d" % (form, N, E, t))
        trace.append(a.t["P"].clone())
    res = b.rollout_fused(T, power_trace=True)
    assert res is not None
    for key in ("Ta", "Tm", "sso", "flags", "P", "reward", "actions"):
        assert torch.equal(a.t[key], b.t[key]), "%s: %s differs between rollout_fused and single steps" % (form, key)
    assert torch.equal(torch.nan_to_num(a.t["obs"], nan=-7.0), torch.nan_to_num(b.t["obs"], nan=-7.0)), form
    assert torch.equal(a.reg_signal(), b.reg_signal()), form
    assert torch.equal(torch.stack(trace), res["power_trace"]), form
    assert torch.equal(rsum, res["reward_sum"]), form
    if ctl == "bangbang":
        return
    for kind in ("always_on", "deadband"):
        b.reset(episode=episode)
        b.set_controller(kind)
        sl = SliceOracle(cfg, b, seed, episode)
        done = 0
        for chunk in (5, 29, 36):          # rollout_fused splits these at the refills (steps 32 and 64)
            near = [np.zeros((sl.k, N), dtype=bool) for _ in sl.oras]
            for _ in range(chunk):
                last = sl.decisions(kind)
                near = [x | y for x, y in zip(near, sl.near_threshold(kind))]
                sl.step(last)
            b.rollout_fused(chunk, accumulate=False)
            done += chunk
            where = "%s (N=%d E=%d) %s, step %d" % (form, N, E, kind, done)
            # the device decides by itself here: a house at a threshold (fp64 within 1e-5 relative) may go the other way and
            # then follows another trajectory - none may on these seeds, and none may anywhere else
            on = [(f & 1).astype(bool) != o.on for f, o in zip(sl.take(b.t["flags"]), sl.oras)]
            n_near, n_far = sum(int((d & m).sum()) for d, m in zip(on, near)), sum(int((d & ~m).sum()) for d, m in zip(on, near))
            assert n_far == 0 and n_near == 0, "%s: %d houses switched otherwise than the oracle away from a threshold, %d at one" % (
                where, n_far, n_near)
            diff, off_edge = sl.decision_misses(sl.take(b.t["actions"]), kind, last)
            assert diff == 0, "%s: %d houses decided otherwise than the oracle (%d away from a threshold)" % (where, diff, off_edge)
            sl.check(b, where)


FILL_HOUSES = 270000


def _fill_case(idx):
    """A device-filling batch of small envs: random N in 1..130, E = ceil(270000 / N) + r, the config drawn as test_gpu_fuzz draws
    it (its own seed streams: the cases of test_gpu_fuzz stay what they are)."""
    from tests.test_gpu_fuzz import _case
    cfg, _, _, seed, episode, p_on, table_steps = _case(200000 + idx)
    rng = np.random.default_rng(41000 + idx)
    N = int(rng.integers(1, 131))
    E = int(math.ceil(FILL_HOUSES / N)) + int(rng.integers(0, 8))
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    return cfg, E, N, seed, episode, p_on, table_steps


@pytest.mark.parametrize("idx", range(32))
def test_device_filling_fuzz_vs_oracle(idx):
    cfg, E, N, seed, episode, p_on, table_steps = _fill_case(idx)
    assert E * N >= pu.DEVICE_FILL
    rw = cfg["default_env_prop"]["reward_prop"]
    scale = max(1.0, float(rw["alpha_temp"]) + float(rw["alpha_sig"]))      # as test_gpu_fuzz
    env = _env(cfg, E, seed, table_steps)
    env.reset(episode=episode)
    sl = SliceOracle(cfg, env, seed, episode, k=3, offsets=[E - 3], r_atol=1e-5 * scale)
    gen = torch.Generator(device="cuda:0").manual_seed(idx)
    where = "fill case %d (N=%d E=%d, %s)" % (idx, N, E, pu.step_kernel(N, E))
    for t in range(24):
        if t % 6 == 5:
            env.step_bangbang()
            acts = sl.take(env.t["actions"])
        else:
            act = (torch.rand((E, N), device="cuda:0", generator=gen) < p_on).to(torch.uint8)
            env.step(act)
            acts = sl.take(act)
        sl.step(acts)
        sl.check(env, "%s step %d" % (where, t), obs=False)
    np.testing.assert_allclose(env.obs_vector("rows")[E - 3:].cpu().numpy(), sl.oras[0].norm_state(cfg), rtol=3e-5, atol=3e-6,
                               err_msg=where)
