"""The resident rollout loops that load a step's row one trip ahead and wait for it behind the step's front (csrc/mdr_resident.hip,
row_arrived / row_ahead): two trips per turn of the loop, the two row registers changing places, an odd trip behind the turns.

    rollout     rollout(K) through the resident path against an env without rollout rows (rollout_rows=False: one interior launch
                per step, the tables) over COMPARED, bit for bit: K in (2, 3, 9, 10, 17, 41) - one trip, a pair of trips, odd and even
                trip counts; 9 x 1024 and 9 x 1000 houses (k_step_fused<4,1,256>, the second with blank lanes), 3 x 260 (<4,1,128>)
                and 5 x 2000 (<4,2,256>, two tiles); bang-bang (the rotated loops) and the deadband controller (the loops that keep
                the load at the top of the trip); one lockout for every house (the stamp loop) and a lockout column (the counter
                loop); at the default capacity and at MDR_ROLLOUT_ROWS=7 - K = 41: launches of 7, 7, 7, 7, 7 and 5 steps.
    group       the group forms, whose rows arrive by per-lane vector loads: k_step_group<32,1> and <8,1>, K in (2, 9, 17), the same
                reference.

A loop that uses a row one step late turns every one of the 10 items red (profiles/r14_README.md section 6).
The knobs are read once per process: every pytest item starts one fresh child (this file run as a script) under its own timeout."""
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
from tests.test_gpu_rollout_resident import RESIDENT_KNOBS, _compare      # noqa: E402
from tests.test_gpu_thermal_pack import CHILD_TIMEOUT, KNOBS      # noqa: E402

TABLE_STEPS = 8
ROWS_KNOB = "MDR_ROLLOUT_ROWS"
UNIFORM_LOCKOUT = 4      # csrc/mdr_step_common.h
SHAPES = {"full": ("k_step_fused<4,1,256>", 1024, 9), "blank": ("k_step_fused<4,1,256>", 1000, 9), "fused128": ("k_step_fused<4,1,128>", 260, 3),
          "tiles2": ("k_step_fused<4,2,256>", 2000, 5), "group32": ("k_step_group<32,1>", 20, 64), "group8": ("k_step_group<8,1>", 7, 64)}
FUSED, GROUP = ("full", "blank", "fused128", "tiles2"), ("group32", "group8")
STEP_COUNTS, GROUP_STEP_COUNTS = (2, 3, 9, 10, 17, 41), (2, 9, 17)
SOURCES = ("bangbang", "deadband")
LOCKOUTS = ("uniform", "column")
CAPS = {"default": ({}, 1024), "rows7": ({ROWS_KNOB: "7"}, 7)}
NOON = "2021-07-15 11:59:10"      # the solar value changes at each minute change
OK = "row-ahead child ok: "


def run_child(environment, *args):
    """One fresh child of this file; returns what it reported.  A child that does not end normally fails the test here."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + RESIDENT_KNOBS + (ROWS_KNOB,)}
    env.update({"MDR_ROLLOUT_RESIDENT_HOUSES": "0"})
    env.update(environment)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    ok = OK + " ".join(str(a) for a in args)
    assert p.returncode == 0 and ok in p.stdout, "%s (rc %s):\n%s" % (args, p.returncode, p.stdout[-4000:])
    return [json.loads(line[len("REPORT "):]) for line in p.stdout.splitlines() if line.startswith("REPORT ")]


def _make(N, E, seed=977, dt=4, temp_mode="noisy_sinusoidal_heatwave", solar=True, lockouts="column", **kw):
    import mdr_amd
    from tests.test_gpu_rollout_rows import _cfg
    cfg = _cfg(N, temp_mode, solar, NOON)
    cfg["default_env_prop"]["time_step"] = dt
    cfg["default_hvac_prop"]["lockout_noise"] = 0 if lockouts == "uniform" else 12
    return mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=TABLE_STEPS, **kw)


def _run_rollout(shape, cap, step_counts):
    import torch
    from tests.test_gpu_rollout_interior import SENTINEL_F, _prefill
    form, N, E = SHAPES[shape]
    assert pu.step_kernel(N, E) == form, (form, N, E, pu.step_kernel(N, E))
    bad, reports = [], []
    for lockouts in LOCKOUTS:
        env = _make(N, E, lockouts=lockouts)
        ref = _make(N, E, lockouts=lockouts, rollout_rows=False)
        env.reset(episode=1)
        assert bool(int(env.t["param_uniform"].item()) & UNIFORM_LOCKOUT) == (lockouts == "uniform"), (shape, lockouts)
        assert env.rollout_resident() and env.rollout_steps_per_launch() == CAPS[cap][1], (shape, env.rollout_steps_per_launch())
        assert not ref.rollout_resident() and ref.rollout_steps_per_launch() == 0 and ref.rollout_plan()[0] >= 0, shape
        for s, source in enumerate(SOURCES):
            env.set_controller(source)
            ref.set_controller(source)
            for K in step_counts:
                label = "%s %s %s K=%d (%s)" % (shape, lockouts, source, K, cap)
                env.reset(episode=1 + s)
                ref.reset(episode=1 + s)
                _prefill(env)
                _prefill(ref)
                env.rollout(K)
                ref.rollout(K)
                torch.cuda.synchronize()
                assert env.steps_taken == ref.steps_taken == K, (label, env.steps_taken, ref.steps_taken)
                _compare(label, env, ref, bad)
                assert not bool((env.t["reward"] == SENTINEL_F).any()), label      # a full last step overwrote every sentinel
        reports.append({"shape": shape, "lockouts": lockouts, "steps_per_launch": env.rollout_steps_per_launch()})
    return reports, bad


def _child():
    mode = sys.argv[1]
    reports, bad = _run_rollout(sys.argv[2], sys.argv[3], STEP_COUNTS if mode == "rollout" else GROUP_STEP_COUNTS)
    for r in reports:
        print("REPORT " + json.dumps(r))
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print(OK + " ".join(sys.argv[1:]))


@pytest.mark.parametrize("cap", sorted(CAPS))
@pytest.mark.parametrize("shape", FUSED)
def test_rollout_with_rows_loaded_a_trip_ahead_equals_the_per_step_interior_path(shape, cap):
    reports = run_child(CAPS[cap][0], "rollout", shape, cap)
    assert [(r["lockouts"], r["steps_per_launch"]) for r in reports] == [(lk, CAPS[cap][1]) for lk in LOCKOUTS]


@pytest.mark.parametrize("shape", GROUP)
def test_group_forms_with_the_rotated_loop_equal_the_per_step_interior_path(shape):
    reports = run_child({}, "group", shape, "default")
    assert [(r["lockouts"], r["steps_per_launch"]) for r in reports] == [(lk, CAPS["default"][1]) for lk in LOCKOUTS]


if __name__ == "__main__":
    _child()
