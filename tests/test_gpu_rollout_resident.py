"""rollout() with the houses resident in registers (k_rollout_resident / k_rollout_resident_group), at every step form the planner can
launch and around the switch that selects it.

By default the resident arm takes batches of 1 << 20 houses and more (MDR_ROLLOUT_RESIDENT_HOUSES); the tests of the interior forms
(tests/test_gpu_rollout_forms.py) run below it and keep reaching the per-step forms.  Here the threshold is set to 0, so the 33 step
forms of tests/plan_util.py::oracle_cases(), each at the smallest batch that selects it, run the resident arm wherever one exists:
the 25 k_step_fused / k_step_group forms; the other eight (k_step_multi, k_step_packed, k_step_single_house, the split step) report
"not resident" and take the path they took.  Configuration, seeds, 8-row tables and the rotation of the action source (bang-bang,
deadband, always-on, external actions) are those of tests/test_gpu_rollout_forms.py.  For every K in (1, 2, 3, 19) rollout(K) must
leave what K single steps on a deep copy leave, bit for bit, over Ta, Tm, sso, flags, actions, reward, P and the seven obs planes,
every output sentinel-filled before the call.  At 8-row tables K = 19 is resident launches of 8, 8 and 2 steps across two refills
and one full step; K = 1 is the full step alone.  The batches include N that are no multiple of the lane footprint (blank houses
in the lanes past the env's end) and a streamed lockout column.

The modes (mdr_env_rollout_plan keeps its answers and is asserted too):
    forms          MDR_ROLLOUT_RESIDENT_HOUSES=0                                    plan (2, not packed): the five columns streamed
    forms_nopack   ... and MDR_THERMAL_PACK=0                                       plan (2, not packed)
    forms_stream   ... and MDR_ROLLOUT_STREAM_HOUSES=0                              plan (0, packed): the benchmark's combination
    switches       one fused and one group batch under each setting of the two knobs (SWITCHES), the constructor's thermal_pack=False,
                   and - after a rollout on the resident arm - a plain step and a state_dict / load_state_dict round trip that go on
                   bit-equal with the twin

The knobs are read once per process: every pytest item starts one fresh child (this file run as a script) under its own timeout,
with the six knobs stripped from the inherited environment and then set for the mode."""
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
from tests.test_gpu_rollout_forms import CASES, CHUNKS, FULL_STEPS, SOURCES, STEP_COUNTS, TABLE_STEPS, has_interior, same_bits      # noqa: E402
from tests.test_gpu_thermal_pack import CHILD_TIMEOUT, KNOBS      # noqa: E402

RESIDENT_KNOBS = ("MDR_ROLLOUT_RESIDENT", "MDR_ROLLOUT_RESIDENT_HOUSES")
# name: (environment, the plan of a k_step_fused / k_step_group batch, chunks)
MODES = {"forms": ({"MDR_ROLLOUT_RESIDENT_HOUSES": "0"}, (2, False), tuple(range(CHUNKS))),
         "forms_nopack": ({"MDR_ROLLOUT_RESIDENT_HOUSES": "0", "MDR_THERMAL_PACK": "0"}, (2, False), (0,)),
         "forms_stream": ({"MDR_ROLLOUT_RESIDENT_HOUSES": "0", "MDR_ROLLOUT_STREAM_HOUSES": "0"}, (0, True), (0,))}
# the switch: (form, N, E) and, per setting, (environment as a function of E * N, constructor arguments, resident?)
SWITCH_CASES = {"fused": ("k_step_fused<4,1,256>", 1024, 8), "group": ("k_step_group<32,1>", 20, 64)}      # group: two envs per wave, 20 of each 32 lanes live
SWITCHES = {"unset": (lambda n: {}, {}, False),
            "at_size": (lambda n: {"MDR_ROLLOUT_RESIDENT_HOUSES": str(n)}, {}, True),
            "above_size": (lambda n: {"MDR_ROLLOUT_RESIDENT_HOUSES": str(n + 1)}, {}, False),
            "off": (lambda n: {"MDR_ROLLOUT_RESIDENT": "0", "MDR_ROLLOUT_RESIDENT_HOUSES": "0"}, {}, False),
            "no_pack_handle": (lambda n: {"MDR_ROLLOUT_RESIDENT_HOUSES": "0"}, {"thermal_pack": False}, True)}


def run_child(environment, *args, script=__file__, ok="resident child ok: "):
    """One fresh child of `script` (this file); returns what it reported.  A child that does not end normally - a time limit, a
    signal, a mismatch - fails the test here, and nothing is started behind it."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + RESIDENT_KNOBS}
    env.update(environment)
    p = subprocess.run([sys.executable, os.path.abspath(script)] + [str(a) for a in args], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    ok = ok + " ".join(str(a) for a in args)
    assert p.returncode == 0 and ok in p.stdout, "%s (rc %s):\n%s" % (args, p.returncode, p.stdout[-4000:])
    return [json.loads(line[len("REPORT "):]) for line in p.stdout.splitlines() if line.startswith("REPORT ")]


def _compare(label, env, ref, bad):
    from tests.test_gpu_rollout_interior import COMPARED
    for k in COMPARED:
        if not same_bits(env.t[k], ref.t[k]):
            bad.append("%s %s: %d of %d elements differ" % (label, k, int((env.t[k] != ref.t[k]).sum()), env.t[k].numel()))


def _actions(E, N, seed):
    import torch
    return (torch.rand((E, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed)) < 0.6).to(torch.uint8)


def _run_form(mode, ic):
    import torch
    from tests.test_gpu_plan_oracle import _cfg, _env
    from tests.test_gpu_rollout_interior import SENTINEL_B, SENTINEL_F, _prefill
    i, (form, N, E, _) = ic
    assert pu.step_kernel(N, E) == form, (form, N, E, pu.step_kernel(N, E))      # the case reaches the form it is there for
    cfg = _cfg(N, i)
    seed, episode = 7919 * i + 13, i % 3
    source = SOURCES[i % len(SOURCES)]
    external = source == "external"
    label = "%s (N=%d E=%d) %s, mode %s" % (form, N, E, source, mode)
    env = _env(cfg, E, seed, TABLE_STEPS)
    env.set_controller("bangbang" if external else source)
    bad = []
    plan, resident = env.rollout_plan(), env.rollout_resident()
    for K in STEP_COUNTS:
        env.reset(episode=episode)
        ref = copy.deepcopy(env)
        _prefill(env)
        _prefill(ref)
        act = _actions(E, N, 1000 * i + K) if external else None
        for t in range(K):
            ref.step(act) if external else ref.step_controller()
        env.rollout(K, act)
        torch.cuda.synchronize()
        assert env.steps_taken == ref.steps_taken == K, (label, K, env.steps_taken, ref.steps_taken)
        _compare("%s K=%d" % (label, K), env, ref, bad)
        if not external:      # a full last step overwrote every sentinel
            assert not bool((env.t["reward"] == SENTINEL_F).any()) and not bool((env.t["actions"] == SENTINEL_B).any()), (label, K)
    return {"i": i, "form": form, "planes": plan[0], "packed": bool(plan[1]), "resident": resident}, bad


def _run_switch(case, setting):
    import torch
    from tests.test_gpu_plan_oracle import _cfg
    from tests.test_gpu_rollout_interior import _prefill
    import mdr_amd
    form, N, E = SWITCH_CASES[case]
    assert pu.step_kernel(N, E) == form, (form, pu.step_kernel(N, E))
    label = "%s (N=%d E=%d), switch %s" % (form, N, E, setting)
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N, 3), nb_envs=E, device="cuda:0", seed=4242, table_steps=TABLE_STEPS, **SWITCHES[setting][1])
    env.reset(episode=1)
    resident = env.rollout_resident()
    bad = []
    ref = copy.deepcopy(env)
    _prefill(env)
    _prefill(ref)
    for t in range(19):
        ref.step_controller()
    env.rollout(19)
    _compare(label + " rollout(19)", env, ref, bad)
    env.step_controller()      # a plain step behind the rollout
    ref.step_controller()
    _compare(label + " step behind the rollout", env, ref, bad)
    sd = env.state_dict()
    env.rollout(3)             # moves on, then back to the snapshot
    env.load_state_dict(sd)
    act = _actions(E, N, 77)
    for t in range(11):
        ref.step(act)
    env.rollout(11, act)
    torch.cuda.synchronize()
    assert env.steps_taken == ref.steps_taken == 31, (label, env.steps_taken, ref.steps_taken)
    _compare(label + " rollout(11, actions) behind load_state_dict", env, ref, bad)
    return {"case": case, "setting": setting, "resident": resident, "plan": list(env.rollout_plan())}, bad


def _chunk(arg):
    return CASES[int(arg)::CHUNKS]


def _child():
    mode = sys.argv[1]
    failed = False
    runs = [(_run_switch, (sys.argv[2], sys.argv[3]))] if mode == "switches" else [(_run_form, (mode, ic)) for ic in _chunk(sys.argv[2])]
    for fn, args in runs:
        report, bad = fn(*args)
        print("REPORT " + json.dumps(report))
        if bad:
            failed = True
            print("\n".join(bad))
    if failed:
        sys.exit(1)
    print("resident child ok: " + " ".join(sys.argv[1:]))


@pytest.mark.parametrize("mode,chunk", [(m, c) for m in sorted(MODES) for c in MODES[m][2]])
def test_resident_rollout_leaves_what_single_steps_leave_at_every_step_form(mode, chunk):
    reports = run_child(MODES[mode][0], mode, chunk)
    cases = _chunk(chunk)
    assert [r["i"] for r in reports] == [i for i, _ in cases]
    for r, (_, (form, N, E, _)) in zip(reports, cases):
        assert r["resident"] == has_interior(form), (form, r)      # the resident arm wherever an interior form exists, nowhere else
        assert (r["planes"], r["packed"]) == (MODES[mode][1] if has_interior(form) else FULL_STEPS), (form, r)      # the plan keeps its answers
    assert sum(r["resident"] for r in reports) == sum(has_interior(c[0]) for _, c in cases)


def test_the_chunks_of_forms_hold_the_25_resident_forms():
    """The census behind the per-chunk assertions above: over its chunks `forms` runs all 33 step forms, 25 of them resident."""
    assert sorted(c for m in ("forms",) for k in MODES[m][2] for c in _chunk(k)) == sorted(CASES) and len(CASES) == 33
    assert sum(has_interior(c[0]) for _, c in CASES) == 25
    assert sum(has_interior(c[0]) for _, c in _chunk(0)) >= 12      # what forms_nopack and forms_stream run


@pytest.mark.parametrize("setting", sorted(SWITCHES))
@pytest.mark.parametrize("case", sorted(SWITCH_CASES))
def test_resident_switches(case, setting):
    form, N, E = SWITCH_CASES[case]
    environment, _, want = SWITCHES[setting]
    (r,) = run_child(environment(N * E), "switches", case, setting)
    assert r["resident"] == want, r
    assert r["plan"] == [2, 0], r      # below MDR_ROLLOUT_STREAM_HOUSES' default: the per-step plan, whatever the resident rule says


if __name__ == "__main__":
    _child()
