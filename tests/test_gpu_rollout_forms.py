"""rollout() at every step form the planner can launch, under each of the four interior plans.

The cases are the 33 step forms of tests/plan_util.py::oracle_cases(), each at the smallest batch that selects it (the device-filling
ones included: up to 262,208 houses), with the configuration of tests/test_gpu_plan_oracle.py (_cfg: the four penalty modes, two
signal families, a streamed lockout column, deadband 0.5) and 8-row tables.  The action source rotates over the case index:
bang-bang, deadband, always-on, external actions.  For every K in (1, 2, 3, 19) - 19 crosses two refills - rollout(K) must leave what
K single steps on a deep copy leave, bit for bit, over Ta, Tm, sso, flags, actions, reward, P and the seven obs planes, every output
sentinel-filled before the call.  25 of the 33 forms are k_step_fused / k_step_group and run their interior instantiation; the other
eight (k_step_multi, k_step_packed, k_step_single_house, the split step) have none: rollout() runs full steps or rollout_split there,
and the plan reads (-1, not packed).

The plans (mdr_env_rollout_plan is read back and asserted):
    default         no knob set                                           (2, not packed) at these sizes
    planes5         MDR_ROLLOUT_INTERIOR_PLANES=5                         (5, not packed)
    stream_nopack   MDR_ROLLOUT_STREAM_HOUSES=0, MDR_THERMAL_PACK=0       (0, not packed)
    stream          MDR_ROLLOUT_STREAM_HOUSES=0                           (0, packed) - the benchmark's plan
Under `stream` the records and the descriptor on the device are also held to the numpy reference (tests/thermal_pack_ref.py), and the
K = 19 run of the single-step twin goes through the fp64 oracle on three slices (tests/slice_oracle.py: controller decisions against
the oracle's rule, every step under its contract) - so what rollout() leaves is bit-equal to single steps that are themselves within
the stated tolerances of fp64.  (The twin does not depend on the knobs: one plan's child is enough.)

What a comparison of values cannot see: an interior instantiation with another LOCAL than the plan's.  LOCAL only says which of the
local planes an interior step still stores, the full last step overwrites every one of them, and no arithmetic hangs on the count -
a dispatch line that passes LOCAL 1 for 2 leaves the same bits (tried on an experiment build) and shows only in the bytes a step moves, that is in its time.  A form whose interior step computes anything differently is seen here.

The knobs are read once per process: every pytest item starts one fresh child (this file run as a script, never an exec) under its own
timeout, with the four knobs stripped from the inherited environment and then set for the plan."""
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
from tests.test_gpu_plan_oracle import STEP_CASES      # noqa: E402
from tests.test_gpu_thermal_pack import CHILD_TIMEOUT, KNOBS      # noqa: E402

STEP_COUNTS = (1, 2, 3, 19)          # table_steps = 8: 19 steps cross two refills
TABLE_STEPS = 8
SOURCES = ("bangbang", "deadband", "always_on", "external")
# name: (environment, the plan of a k_step_fused / k_step_group batch)
PLANS = {"default": ({}, (2, False)),
         "planes5": ({"MDR_ROLLOUT_INTERIOR_PLANES": "5"}, (5, False)),
         "stream_nopack": ({"MDR_ROLLOUT_STREAM_HOUSES": "0", "MDR_THERMAL_PACK": "0"}, (0, False)),
         "stream": ({"MDR_ROLLOUT_STREAM_HOUSES": "0"}, (0, True))}
FULL_STEPS = (-1, False)             # what the plan reads where the step form has no interior instantiation
CASES = STEP_CASES                   # (index in oracle_cases(), (form, N, E, None)): the 33 step forms
CHUNKS = 2                           # chunk c holds CASES[c::CHUNKS]: the device-filling batches spread over the chunks


def has_interior(form):
    return form.startswith(("k_step_fused<", "k_step_group<"))


def run_child(script, plan, arg):
    """One fresh child of `script` under `plan`; returns what it reported (a dict per case).  A child that does not end normally -
    a time limit, a signal, a mismatch - fails the test here, and nothing is started behind it."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(PLANS[plan][0])
    p = subprocess.run([sys.executable, os.path.abspath(script), plan, str(arg)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    ok = "rollout child ok: %s %s" % (plan, arg)
    assert p.returncode == 0 and ok in p.stdout, "%s %s (rc %s):\n%s" % (plan, arg, p.returncode, p.stdout[-4000:])
    reports = [json.loads(line[len("REPORT "):]) for line in p.stdout.splitlines() if line.startswith("REPORT ")]
    return reports


def child_main(run_case, cases_of):
    """The child's side: run_case(plan, case) -> (report dict, list of mismatches) for every case of the chunk."""
    plan, arg = sys.argv[1], sys.argv[2]
    failed = False
    for case in cases_of(arg):
        report, bad = run_case(plan, case)
        print("REPORT " + json.dumps(report))
        if bad:
            failed = True
            print("\n".join(bad))
    if failed:
        sys.exit(1)
    print("rollout child ok: %s %s" % (plan, arg))


def same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.numel() else a.numel() == b.numel()      # bits, so that NaN == NaN


def _run_case(plan, ic):
    import torch
    from tests.slice_oracle import SliceOracle
    from tests.test_gpu_plan_oracle import _cfg, _controller_run, _env
    from tests.test_gpu_rollout_interior import COMPARED, SENTINEL_B, SENTINEL_F, _prefill
    from tests.test_gpu_thermal_pack import _device_pack, _pack_matches
    from mdr_amd import _native as nat
    i, (form, N, E, _) = ic
    assert pu.step_kernel(N, E) == form, (form, N, E, pu.step_kernel(N, E))      # the case reaches the form it is there for
    cfg = _cfg(N, i)
    seed, episode = 7919 * i + 13, i % 3
    source = SOURCES[i % len(SOURCES)]
    external = source == "external"
    label = "%s (N=%d E=%d) %s, plan %s" % (form, N, E, source, plan)
    env = _env(cfg, E, seed, TABLE_STEPS)
    env.set_controller("bangbang" if external else source)
    bad = []
    want = PLANS[plan][1] if has_interior(form) else FULL_STEPS
    got = env.rollout_plan()
    if got != want:
        bad.append("%s: plan %s, expected %s" % (label, got, want))
    for K in STEP_COUNTS:
        env.reset(episode=episode)
        ref = copy.deepcopy(env)
        _prefill(env)
        _prefill(ref)
        act = None
        if external:
            act = (torch.rand((E, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1000 * i + K)) < 0.6).to(torch.uint8)
        sl = SliceOracle(cfg, ref, seed, episode) if plan == "stream" and K == STEP_COUNTS[-1] else None
        for t in range(K):
            where = "%s, single step %d of %d" % (label, t, K)
            if sl is None:
                ref.step(act) if external else ref.step_controller()
            elif external:
                ref.step(act)
                sl.step(sl.take(act))
                sl.check(ref, where)
            else:
                _controller_run(ref, sl, source, where)      # decisions against the oracle's rule (off_edge == 0), sl.check
        env.rollout(K, act)
        torch.cuda.synchronize()
        assert env.steps_taken == ref.steps_taken == K, (label, K, env.steps_taken, ref.steps_taken)
        for k in COMPARED:
            if not same_bits(env.t[k], ref.t[k]):
                bad.append("%s K=%d %s: %d of %d elements differ" % (label, K, k, int((env.t[k] != ref.t[k]).sum()), env.t[k].numel()))
        if not external:      # a full last step overwrote every sentinel
            assert not bool((env.t["reward"] == SENTINEL_F).any()) and not bool((env.t["actions"] == SENTINEL_B).any()), (label, K)
    desc_word = None
    if plan == "stream":
        # big_noise houses at the default time step fit their fields (tests/test_thermal_pack.py: the corners of the noise box)
        bad += _pack_matches(label, env)
        desc_word = int(_device_pack(env)[0][nat.MDR_THERMAL_DESC_PACKED])
    return {"i": i, "form": form, "planes": got[0], "packed": bool(got[1]), "desc": desc_word}, bad


def _chunk(arg):
    return CASES[int(arg)::CHUNKS]


@pytest.mark.parametrize("chunk", range(CHUNKS))
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_rollout_leaves_what_single_steps_leave_at_every_step_form(plan, chunk):
    reports = run_child(__file__, plan, chunk)
    cases = _chunk(chunk)
    assert [r["i"] for r in reports] == [i for i, _ in cases]
    for r, (_, (form, N, E, _)) in zip(reports, cases):
        want = PLANS[plan][1] if has_interior(form) else FULL_STEPS
        assert (r["planes"], r["packed"]) == want, (form, r)
        if plan == "stream":
            assert r["desc"] == 1, (form, r)
    # every fused / group form of the chunk ran its interior instantiation (over the chunks: 25 of the 33)
    assert sum(r["planes"] >= 0 for r in reports) == sum(has_interior(c[0]) for _, c in cases)


if __name__ == "__main__":
    child_main(_run_case, _chunk)
