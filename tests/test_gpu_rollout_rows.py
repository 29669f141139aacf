"""The rollout rows (mdr_env_bind_rollout_rows, csrc/mdr_rollout_rows.hip): the two table values per env and step that a resident
launch of rollout() reads, built in front of the launch for as many steps as it runs - so that a launch ends with the rows' capacity,
not with the time tables.

Three batches, the threshold at 0 (MDR_ROLLOUT_RESIDENT_HOUSES=0) and 8-row tables throughout: the benchmark's fused form (N = 1024,
E = 8), a fused form with blank lanes (N = 260: 65 of 128 lanes hold houses) and a group form (N = 20, E = 64: two envs per wave, 12 idle
lanes per env).

    rows        mdr_env_fill_rollout_rows for 40 rows from k = 0 and from k = 13 against tab_od / tab_solar read row by row, at the
                cursor, while the env is stepped through seven 8-row windows: row r of a fill from k is {tab_od at time index k + r,
                tab_solar at k + r + 1}, bit for bit - in each of ROW_CONFIGS, and the same again after the cursor moved
    steps       rollout(K) against K single steps on a deep copy for K in (2, 9, 10, 19, 70) over COMPARED, outputs sentinel-filled,
                all four action sources; at the default capacity (every K one launch) and at MDR_ROLLOUT_ROWS=5 (K = 19: launches of
                5, 5, 5, 3; K = 70: fourteen)
    after       behind rollout(70): a plain step, rollout(3), a state_dict / rollout / load_state_dict round trip, reset(episode + 1)
                then rollout(19), and rollout(19) after a seed change - each bit-equal with the stepped twin
    capacity    the steps-per-launch rule, no GPU work beyond creating envs: the byte budget at large E, time_step x steps < 2^31,
                0 without the buffer

The knobs are read once per process: every pytest item starts one fresh child (this file run as a script) under its own timeout."""
import copy
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import plan_util as pu      # noqa: E402
from tests.test_gpu_rollout_forms import SOURCES, same_bits      # noqa: E402
from tests.test_gpu_rollout_resident import RESIDENT_KNOBS, _actions, _compare      # noqa: E402
from tests.test_gpu_thermal_pack import CHILD_TIMEOUT, KNOBS      # noqa: E402

TABLE_STEPS = 8
ROWS_KNOB = "MDR_ROLLOUT_ROWS"
BATCHES = {"fused": ("k_step_fused<4,1,256>", 1024, 8), "blank": ("k_step_fused<4,1,128>", 260, 3), "group": ("k_step_group<32,1>", 20, 64)}
STEP_COUNTS = (2, 9, 10, 19, 70)
NROWS, STARTS = 40, (0, 13)
# name: (temp_mode, solar gain, fixed start or None = random, rows of a recorded outdoor-temperature table)
ROW_CONFIGS = {"std_zero": ("shifting_sinusoidal_heatwave", True, None, 0),           # temp_std == 0: no draw; random phase
               "std_nonzero": ("noisier_sinusoidal_heatwave", True, None, 0),          # the TAG_OD_NOISE Gaussian at every row
               "solar_off": ("noisy_sinusoidal_heatwave", False, "2021-07-15 11:58:50", 0),
               "solar_on": ("noisy_sinusoidal_heatwave", True, "2021-07-15 11:58:50", 0),   # noon: the solar value changes at each of the 3 - 4 minute changes
               "midnight": ("noisy_sinusoidal_heatwave", True, "2021-06-30 23:58:30", 0),  # 40 rows of 4 s: 23:58:30 .. 00:01:10, over the day's and the month's end
               "od_table": ("noisy_sinusoidal_heatwave", True, None, 10)}              # rows 0 - 9 from the table, row 10 on from the sinusoid
CAPS = {"default": ({}, 1024), "rows5": ({ROWS_KNOB: "5"}, 5)}


def run_child(environment, *args):
    """One fresh child of this file; returns what it reported.  A child that does not end normally fails the test here."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + RESIDENT_KNOBS + (ROWS_KNOB,)}
    env.update({"MDR_ROLLOUT_RESIDENT_HOUSES": "0"})
    env.update(environment)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    ok = "rows child ok: " + " ".join(str(a) for a in args)
    assert p.returncode == 0 and ok in p.stdout, "%s (rc %s):\n%s" % (args, p.returncode, p.stdout[-4000:])
    return [json.loads(line[len("REPORT "):]) for line in p.stdout.splitlines() if line.startswith("REPORT ")]


def _cfg(N, temp_mode="noisy_sinusoidal_heatwave", solar=True, start=None):
    from tests.test_gpu_plan_oracle import _cfg as base
    cfg = base(N, 3)
    cfg["default_env_prop"]["cluster_prop"]["temp_mode"] = temp_mode
    cfg["default_house_prop"]["solar_gain_bool"] = bool(solar)
    if start is not None:
        cfg["default_env_prop"]["start_datetime_mode"] = "fixed"
        cfg["default_env_prop"]["start_datetime"] = start
    return cfg


def _make(batch, cfg=None, seed=4242, **kw):
    import mdr_amd
    form, N, E = BATCHES[batch]
    assert pu.step_kernel(N, E) == form, (form, pu.step_kernel(N, E))
    return mdr_amd.BatchedDemandResponseEnv(cfg if cfg is not None else _cfg(N), nb_envs=E, device="cuda:0", seed=seed, table_steps=TABLE_STEPS, **kw)


def _run_rows(name):
    import numpy as np
    import torch
    temp_mode, solar, start, od_rows = ROW_CONFIGS[name]
    bad, reports = [], []
    for batch, (form, N, E) in BATCHES.items():
        env = _make(batch, _cfg(N, temp_mode, solar, start), seed=977)
        env.reset(episode=2)
        if od_rows:
            tab = 30.0 + 5.0 * np.random.default_rng(5).random((od_rows, E))
            env.set_od_table(tab)
            env._begin_episode()      # the tables of the first window again, from the recorded rows
        assert (env.spec.temp_std == 0.0) == (name == "std_zero") and env.spec.solar_gain == solar
        fills = {k: env.fill_rollout_rows(k, NROWS) for k in STARTS}      # at cursor 0: a fill reads neither tables nor cursor
        od, sol = [], []
        last = max(STARTS) + NROWS
        for k in range(last + 1):      # time indices 0 .. last: the rows at the cursor, window after window
            assert env.steps_taken == k and 0 <= env._row() <= TABLE_STEPS
            od.append(env.table("tab_od")[env._row()].clone())
            sol.append(env.table("tab_solar")[env._row()].clone())
            env.step_controller()
        od, sol = torch.stack(od), torch.stack(sol)
        if od_rows:
            want = (torch.as_tensor(tab, device="cuda:0") - env.spec.temp_ref).float()
            assert same_bits(od[:od_rows], want), "the recorded outdoor temperatures did not reach the tables"
            assert not same_bits(od[od_rows], od[od_rows - 1])
        for k in STARTS:
            again = env.fill_rollout_rows(k, NROWS)      # the cursor has moved on: the same rows
            for label, got in (("fill", fills[k]), ("fill behind %d steps" % (last + 1), again)):
                got_od, got_sol = got[:, :, 0].contiguous(), got[:, :, 1].contiguous()
                if not same_bits(got_od, od[k:k + NROWS]):
                    bad.append("%s %s %s from k=%d: od differs in %d of %d" % (name, batch, label, k, int((got_od != od[k:k + NROWS]).sum()), NROWS * E))
                if not same_bits(got_sol, sol[k + 1:k + 1 + NROWS]):
                    bad.append("%s %s %s from k=%d: solar differs in %d of %d" % (name, batch, label, k, int((got_sol != sol[k + 1:k + 1 + NROWS]).sum()), NROWS * E))
        reports.append({"batch": batch, "solar_values": int(torch.unique(sol[:NROWS + 1]).numel()), "od_values": int(torch.unique(od[:NROWS]).numel())})
    return reports, bad


def _twin_steps(ref, K, act):
    for _ in range(K):
        ref.step(act) if act is not None else ref.step_controller()


def _run_steps(cap):
    import torch
    from tests.test_gpu_rollout_interior import SENTINEL_B, SENTINEL_F, _prefill
    bad, reports = [], []
    for b, (batch, (form, N, E)) in enumerate(BATCHES.items()):
        env = _make(batch)
        assert env.rollout_resident() and env.rollout_steps_per_launch() == CAPS[cap][1], (batch, env.rollout_steps_per_launch())
        for s, source in enumerate(SOURCES):
            external = source == "external"
            env.set_controller("bangbang" if external else source)
            for K in STEP_COUNTS:
                label = "%s %s K=%d (%s)" % (batch, source, K, cap)
                env.reset(episode=(b + s) % 3)
                ref = copy.deepcopy(env)
                _prefill(env)
                _prefill(ref)
                act = _actions(E, N, 100 * s + K) if external else None
                _twin_steps(ref, K, act)
                env.rollout(K, act)
                torch.cuda.synchronize()
                assert env.steps_taken == ref.steps_taken == K, (label, env.steps_taken, ref.steps_taken)
                assert 0 <= env._row() <= TABLE_STEPS, (label, env.cursor())      # the full last step left the cursor inside the tables
                _compare(label, env, ref, bad)
                if not external:      # a full last step overwrote every sentinel
                    assert not bool((env.t["reward"] == SENTINEL_F).any()) and not bool((env.t["actions"] == SENTINEL_B).any()), label
        reports.append({"batch": batch, "steps_per_launch": env.rollout_steps_per_launch(), "resident": env.rollout_resident()})
    return reports, bad


def _run_after(_):
    import torch
    from tests.test_gpu_rollout_interior import _prefill
    bad, reports = [], []
    for batch, (form, N, E) in BATCHES.items():
        env = _make(batch)
        env.reset(episode=1)
        assert env.rollout_resident() and env.rollout_steps_per_launch() >= 70
        ref = copy.deepcopy(env)
        _prefill(env)
        _prefill(ref)
        env.rollout(70)      # one launch of 69 steps over eight table windows, then the full step
        _twin_steps(ref, 70, None)
        _compare(batch + " rollout(70)", env, ref, bad)
        assert env.cursor()[0] == 70 and 0 <= env._row() <= TABLE_STEPS, env.cursor()
        if not same_bits(env.reg_signal(), ref.reg_signal()) or not same_bits(env.od_temp(), ref.od_temp()):
            bad.append(batch + ": the table rows at the cursor differ behind rollout(70)")
        env.step_controller()
        ref.step_controller()
        _compare(batch + " a plain step behind it", env, ref, bad)
        env.rollout(3)
        _twin_steps(ref, 3, None)
        _compare(batch + " rollout(3) behind it", env, ref, bad)
        sd = env.state_dict()
        env.rollout(21)      # moves on, then back to the snapshot
        env.load_state_dict(sd)
        act = _actions(E, N, 77)
        env.rollout(19, act)
        _twin_steps(ref, 19, act)
        _compare(batch + " rollout(19, actions) behind load_state_dict", env, ref, bad)
        env.reset(episode=2)
        ref.reset(episode=2)
        env.rollout(19)
        _twin_steps(ref, 19, None)
        _compare(batch + " rollout(19) behind reset(episode + 1)", env, ref, bad)
        env.reset(seed=99, episode=2)
        ref.reset(seed=99, episode=2)
        env.rollout(19)
        _twin_steps(ref, 19, None)
        torch.cuda.synchronize()
        assert env.steps_taken == ref.steps_taken == 19
        _compare(batch + " rollout(19) behind a seed change", env, ref, bad)
        reports.append({"batch": batch})
    return reports, bad


def _run_capacity(_):
    import mdr_amd
    from mdr_amd import _native as nat
    lib = nat.load()
    budget = 64 << 20
    out = {}
    env = _make("group")
    out["default"] = [env.rollout_steps_per_launch(), list(env.t["rollout_rows"].shape), env.rollout_resident()]
    big_e = 9000       # 8 B per env and row: 932 rows fit 64 MiB (still k_step_group<32,1>: beyond ~10,000 envs of 20 the plan is k_step_packed)
    assert pu.step_kernel(20, big_e) == BATCHES["group"][0]
    big = mdr_amd.BatchedDemandResponseEnv(_cfg(20), nb_envs=big_e, device="cuda:0", seed=1, table_steps=TABLE_STEPS)
    out["big"] = [big.rollout_steps_per_launch(), list(big.t["rollout_rows"].shape), big.rollout_resident()]
    assert big.t["rollout_rows"].numel() * 4 <= budget < (big.t["rollout_rows"].shape[0] + 1) * big_e * 8
    out["rows"] = {str(e): int(lib.mdr_rollout_rows(e)) for e in (0, 1, 8184, 8192, 209715, 1 << 24)}
    for dt, want in ((3000000, ((1 << 31) - 1) // 3000000), (1 << 30, 1)):
        cfg = _cfg(20)
        cfg["default_env_prop"]["time_step"] = dt
        slow = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=64, device="cuda:0", seed=1, table_steps=TABLE_STEPS)
        steps = slow.rollout_steps_per_launch()
        assert steps == want and dt * steps < 1 << 31 <= dt * (steps + 1), (dt, steps)
        out["dt_%d" % dt] = [steps, slow.rollout_resident()]
    none = _make("group", rollout_rows=False)
    out["unbound"] = [none.rollout_steps_per_launch(), "rollout_rows" in none.t, none.rollout_resident(), list(none.rollout_plan())]
    out["bound_plan"] = list(env.rollout_plan())
    return [out], []


def _child():
    mode, arg = sys.argv[1], sys.argv[2]
    reports, bad = {"rows": _run_rows, "steps": _run_steps, "after": _run_after, "capacity": _run_capacity}[mode](arg)
    for r in reports:
        print("REPORT " + json.dumps(r))
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print("rows child ok: " + " ".join(sys.argv[1:]))


@pytest.mark.parametrize("name", sorted(ROW_CONFIGS))
def test_rollout_rows_equal_the_table_rows(name):
    reports = run_child({}, "rows", name)
    assert [r["batch"] for r in reports] == list(BATCHES)
    for r in reports:      # the configuration did what it is there for: the values change along the rows (solar: at noon; never when off or at night)
        assert r["od_values"] > 1, r
        if name in ("solar_off", "solar_on", "midnight"):
            assert (r["solar_values"] > 1) == (name == "solar_on"), r


@pytest.mark.parametrize("cap", sorted(CAPS))
def test_rollout_equals_single_steps_at_every_capacity(cap):
    reports = run_child(CAPS[cap][0], "steps", cap)
    assert [(r["batch"], r["steps_per_launch"], r["resident"]) for r in reports] == [(b, CAPS[cap][1], True) for b in BATCHES]


def test_what_follows_a_long_launch_stays_bit_equal():
    assert [r["batch"] for r in run_child({}, "after", "all")] == list(BATCHES)


def test_steps_per_launch_obey_the_byte_budget_and_the_blank_lane_rule():
    (r,) = run_child({}, "capacity", "all")
    assert r["default"] == [1024, [1025, 64, 2], True], r
    assert r["big"] == [(64 << 20) // (8 * 9000) - 1, [(64 << 20) // (8 * 9000), 9000, 2], True] and r["big"][0] == 931, r
    assert r["rows"] == {"0": 0, "1": 1025, "8184": 1025, "8192": 1024, "209715": 40, str(1 << 24): 2}, r
    assert r["dt_3000000"] == [715, True] and r["dt_%d" % (1 << 30)] == [1, True], r
    assert r["unbound"] == [0, False, False, r["bound_plan"]], r      # without the buffer: one launch per interior step, the plan's answers unchanged


if __name__ == "__main__":
    _child()
