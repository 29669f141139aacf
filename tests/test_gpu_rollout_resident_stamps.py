"""The time-stamp loop of the resident rollout kernels (csrc/mdr_resident.hip: house_advance_stamp_m under one lockout for every
house) against single steps, bit for bit.  tests/test_stamp_step_algebra.py checks the integer algebra on the CPU; here rollout(K)
on the resident arm (MDR_ROLLOUT_RESIDENT_HOUSES=0) must leave what K single steps on a deep-copied twin leave over the tensors
tests/test_gpu_rollout_resident.py compares, every output sentinel-filled before the call, and one further plain step behind every
rollout must agree again: the epilogue's sso and lock bit feed the next kernel.  The runs are placed on the solar value's minute
edges - where a loop that holds anything derived from it over the steps of a minute would go wrong - and at night, sunrise and sunset.
8-row tables, dt = 4 s, one fresh child per item.

Shapes (tests/test_gpu_rollout_resident_lean.py): k_step_fused<4,1,256> at N = 1024, E = 8; k_step_fused<4,1,128> at N = 260 (blank
lanes); k_step_group<32,1> at N = 20, E = 64 (two envs per wave, each lane its own env's rows).

entry   lockout_noise = 0: one lockout L = 40 s = 10 dt for every house, no column streamed - the UNIFORM_LOCKOUT bit of param_uniform
        is asserted - or lockout_noise = 12: a streamed column, the counter loop.  The state handed in through load_state_dict holds
        houses on with sso in {1, dt, L - dt, L, L + dt} and off with sso in {0, L - 2 dt, L - dt, L, 10^6}, each with the lock bit
        clear and set.  From 11:59:10 on a July day, K in (2, 3, 17, 40): 17 steps cross one minute edge inside the launch, 40 two,
        and the solar value changes at each.  Bang-bang and external actions on every shape and with either lockout, the controllers
        on fused256 (whose controller instantiation holds the counter body alone: the bit then changes nothing, which is checked too).
solar   Uniform lockout, the state a reset leaves, bang-bang and external actions, K in (17, 40), all three shapes per child.  The start
        is placed from the rows themselves (a day of fill_rollout_rows from midnight): `night` (solar 0 throughout), `sunrise` and
        `sunset` (0 -> non-zero and back at the minute edge eight steps into the launch), `daylight`, `solar_off` (no solar gain),
        `random` (group32 only: a random start per env, so the lanes of one wave read different solar values and change minute at
        different steps) and `mid_minute` (daylight at MDR_ROLLOUT_ROWS=5: launches of 5 steps, all but the first start inside
        a minute)."""
import copy
import datetime
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_rollout_resident import SOURCES, TABLE_STEPS, _actions, _compare, run_child      # noqa: E402
from tests.test_gpu_rollout_resident_lean import ENVIRONMENT, SHAPES      # noqa: E402
from tests import plan_util as pu      # noqa: E402

UNIFORM_LOCKOUT = 4      # csrc/mdr_step_common.h
STEP_COUNTS = (2, 3, 17, 40)
SOLAR_STEP_COUNTS = (17, 40)
NOON = "2021-07-15 11:59:10"
MIDNIGHT = "2021-07-15 00:00:00"
EDGE_STEP = 8      # where `sunrise` / `sunset` put the solar edge inside a launch
FAR = 10 ** 6
ENTRY_ITEMS = ([("fused256", s, "uniform") for s in SOURCES] + [(shape, s, "uniform") for shape in ("fused128", "group32") for s in ("bangbang", "external")]
               + [(shape, s, "column") for shape in sorted(SHAPES) for s in ("bangbang", "external")])
SOLAR_ITEMS = ("night", "sunrise", "sunset", "daylight", "solar_off", "random", "mid_minute")
OK = "stamps child ok: "


def _make(shape, lockouts="uniform", solar=True, start=NOON, seed=977):
    from tests.test_gpu_plan_oracle import _env
    from tests.test_gpu_rollout_rows import _cfg
    form, N, E = SHAPES[shape]
    assert pu.step_kernel(N, E) == form, (form, N, E, pu.step_kernel(N, E))
    cfg = _cfg(N, solar=solar, start=start)
    cfg["default_hvac_prop"]["lockout_noise"] = 0 if lockouts == "uniform" else 12
    env = _env(cfg, E, seed, TABLE_STEPS)
    env.reset(episode=1)
    assert env.rollout_resident() and int(env.spec.time_step) == 4, shape
    word = int(env.t["param_uniform"].item())
    assert bool(word & UNIFORM_LOCKOUT) == (lockouts == "uniform"), (shape, lockouts, word)
    return env, N, E


def _rollout_and_a_step(label, env, ref, K, act, bad):
    """rollout(K) against K single steps, then one plain step on both."""
    import torch
    from tests.test_gpu_rollout_interior import _prefill
    _prefill(env)
    _prefill(ref)
    for t in range(K):
        ref.step(act) if act is not None else ref.step_controller()
    env.rollout(K, act)
    torch.cuda.synchronize()
    assert env.steps_taken == ref.steps_taken, (label, env.steps_taken, ref.steps_taken)
    _compare(label, env, ref, bad)
    for e in (env, ref):
        e.step(act) if act is not None else e.step_controller()
    torch.cuda.synchronize()
    _compare(label + " and a step", env, ref, bad)


def _run_entry(shape, source, lockouts):
    import torch
    from tests.test_gpu_rollout_resident_lean import _house_index
    env, N, E = _make(shape, lockouts)
    external = source == "external"
    env.set_controller("bangbang" if external else source)
    dt = int(env.spec.time_step)
    L = env.t["lockout"].clone()
    assert (int(L.min()) == int(L.max())) == (lockouts == "uniform") and int(L.max()) >= 2 * dt
    on_sso = (torch.ones_like(L), torch.full_like(L, dt), L - dt, L, L + dt)
    off_sso = (torch.zeros_like(L), L - 2 * dt, L - dt, L, torch.full_like(L, FAR))
    patterns = [(1, s, lock) for s in on_sso for lock in (0, 2)] + [(0, s, lock) for s in off_sso for lock in (0, 2)]
    pick = _house_index(env) % len(patterns)
    for j, (on, sso, lock) in enumerate(patterns):
        m = pick == j
        env.t["sso"][m] = sso.clamp(min=0)[m].to(env.t["sso"].dtype)
        env.t["flags"][m] = on | lock
    broken = int(((env.t["flags"] & 1) != 0).logical_and(env.t["sso"] != 0).sum())      # `on` houses that arrive with a count
    far = int(((env.t["flags"] & 1) == 0).logical_and(env.t["sso"] >= FAR).sum())      # houses off for longer than any lockout
    sd = env.state_dict()
    ref = copy.deepcopy(env)
    rows = env.fill_rollout_rows(0, max(STEP_COUNTS))[:, 0, 1]
    edges = [int((rows[1:K] != rows[:K - 1]).sum()) for K in STEP_COUNTS]      # solar changes between the rows of a launch of K - 1 steps
    bad = []
    for K in STEP_COUNTS:
        for e in (env, ref):
            e.load_state_dict(sd)
        act = _actions(E, N, 31 * K) if external else None
        _rollout_and_a_step("%s %s %s entry K=%d" % (shape, source, lockouts, K), env, ref, K, act, bad)
    return {"on_with_sso": broken, "far": far, "edges": edges}, bad


def _solar_of_a_day(shape):
    """The solar value of every 4 s step of the day from midnight (env 0; one fixed start for all), as a CPU tensor."""
    import torch
    env, _, _ = _make(shape, start=MIDNIGHT)
    chunk, day = 900, 24 * 3600 // 4
    return torch.cat([env.fill_rollout_rows(k, min(chunk, day - k))[:, 0, 1].cpu() for k in range(0, day, chunk)])


def _start_at(step):
    """The start that puts time index `step` of the day from midnight EDGE_STEP steps into a rollout."""
    t = datetime.datetime.strptime(MIDNIGHT, "%Y-%m-%d %H:%M:%S") + datetime.timedelta(seconds=4 * (step - EDGE_STEP))
    return t.strftime("%Y-%m-%d %H:%M:%S")


def _run_solar(when):
    import torch
    solar, start = when != "solar_off", NOON
    if when in ("night", "sunrise", "sunset"):
        day = _solar_of_a_day("fused128")
        lit = (day != 0).nonzero().flatten()
        first, last = int(lit[0]), int(lit[-1])
        assert first > 400 and last < day.numel() - 100 and first % 15 == 14 and last % 15 == 13, (first, last)      # row r holds the solar of time index r + 1: a minute edge
        start = {"night": _start_at(first - 300), "sunrise": _start_at(first), "sunset": _start_at(last + 1)}[when]
    elif when == "random":
        start = None
    bad, seen = [], {}
    for shape in (("group32",) if when == "random" else sorted(SHAPES)):
        env, N, E = _make(shape, solar=solar, start=start)
        rows = env.fill_rollout_rows(0, max(SOLAR_STEP_COUNTS))[:, :, 1]      # [row][env]
        changes = (rows[1:] != rows[:-1])
        seen[shape] = {"zero_first": bool((rows[0] == 0).all()), "zero_last": bool((rows[-1] == 0).all()), "all_zero": bool((rows == 0).all()),
                       "edges_min": int(changes.sum(0).min()), "edge_patterns": int(torch.unique(changes.t().to(torch.uint8), dim=0).shape[0]),
                       "waves_with_two_edge_patterns": int((changes[:, 0::2] != changes[:, 1::2]).any(0).sum()),      # envs 2 w and 2 w + 1 share wave w of group32
                       "launch": env.rollout_steps_per_launch()}
        for s, source in enumerate(("bangbang", "external")):
            env.set_controller("bangbang")
            for K in SOLAR_STEP_COUNTS:
                env.reset(episode=1 + s)
                ref = copy.deepcopy(env)
                act = _actions(E, N, 7 * K + s) if source == "external" else None
                _rollout_and_a_step("%s %s %s K=%d" % (when, shape, source, K), env, ref, K, act, bad)
    return seen, bad


def _child():
    kind = sys.argv[1]
    report, bad = _run_entry(*sys.argv[2:5]) if kind == "entry" else _run_solar(sys.argv[2])
    print("REPORT " + json.dumps(report))
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print(OK + " ".join(sys.argv[1:]))


@pytest.mark.parametrize("shape,source,lockouts", ENTRY_ITEMS)
def test_entry_states_minute_edges_and_a_step_behind(shape, source, lockouts):
    (r,) = run_child(ENVIRONMENT, "entry", shape, source, lockouts, script=__file__, ok=OK)
    assert r["on_with_sso"] > 0 and r["far"] > 0, r      # the hand-in broke `on => sso == 0`, and a house off for 10^6 s stayed off
    assert r["edges"] == [0, 0, 1, 2], r      # K = 17 crosses one minute edge inside its launch, K = 40 two, the solar bits change at each


@pytest.mark.parametrize("when", SOLAR_ITEMS)
def test_solar_runs(when):
    environment = dict(ENVIRONMENT, MDR_ROLLOUT_ROWS="5") if when == "mid_minute" else ENVIRONMENT
    (seen,) = run_child(environment, "solar", when, script=__file__, ok=OK)
    assert sorted(seen) == (["group32"] if when == "random" else sorted(SHAPES)), seen
    for shape, r in seen.items():      # the start did what it is there for
        assert r["launch"] == (5 if when == "mid_minute" else 1024), (shape, r)
        if when in ("night", "solar_off"):
            assert r["all_zero"], (shape, r)
        elif when == "sunrise":
            assert r["zero_first"] and not r["zero_last"], (shape, r)
        elif when == "sunset":
            assert not r["zero_first"] and r["zero_last"], (shape, r)
        elif when == "random":
            assert r["waves_with_two_edge_patterns"] > 0 and r["edge_patterns"] > 2, (shape, r)      # lanes of one wave change minute at different steps
        else:
            assert r["edges_min"] >= 2 and not r["zero_first"], (shape, r)


if __name__ == "__main__":
    _child()
