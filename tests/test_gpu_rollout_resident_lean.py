"""The lean loop of the resident rollout kernels (csrc/mdr_resident.hip: house_advance_lean_m, house_lock_m) at the states and steps
where it differs from the per-step update: entry states that break `on => sso == 0`, and the lock bit, which the kernel forms once
behind the last step of a launch.  tests/test_lean_step_algebra.py checks the algebra on the CPU; here rollout(K) on the resident
arm (MDR_ROLLOUT_RESIDENT_HOUSES=0) must leave what K single steps on a twin leave, bit for bit over the tensors
tests/test_gpu_rollout_resident.py compares, every output sentinel-filled before the call.  8-row tables; one fresh child per item.

Shapes: k_step_fused<4,1,256> at N = 1024, E = 8 (the benchmark's instantiation, every lane live), k_step_fused<4,1,128> at N = 260
(blank lanes in the tile), k_step_group<32,1> at N = 20, E = 64 (two envs per wave, 12 blank lanes each).

entry   Written into the state and handed in through load_state_dict: houses with the HVAC on and sso in {1, dt, L - dt, L, L + dt},
        houses off with sso in {0, L - 2 dt, L - dt, L} (L the house's own lockout, a streamed column; negative values clamped
        to 0), each with the lock bit clear and set.  The first step of every launch must therefore run the general form.
        K in (2, 3, 9, 19): one interior step, two (the second in the lean form), a whole 8-row window, and launches of 8, 8, 2.
        All four action sources on the fused shape (the bang-bang and the controller instantiation), bang-bang and external
        actions on the other two.
lock    Lockouts of 0, dt, 2 dt, 5 dt by house (a streamed column) or 5 dt for every house (no column).  The actions buffer of a
        rollout is one constant mask, so a switch is placed by the entry state:
          on   every house off, commanded on, with sso = max(0, L - (K - 1) dt): `can` turns true in interior step K - 2, the
               last one, wherever L >= (K - 1) dt (every house under the uniform lockout), at the house's earliest step elsewhere;
          off  every house on, commanded off: it goes off in step 0 - at K = 2 the last interior step - and the lock bit then
               holds for the house's lockout.
        K in (2, 3, 6).  After rollout(K), and again after a further plain step, flags and the hvac_lockout obs plane (all of
        COMPARED) equal the twin's."""
import copy
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_rollout_resident import SOURCES, TABLE_STEPS, _actions, _compare, run_child      # noqa: E402
from tests import plan_util as pu      # noqa: E402

ENVIRONMENT = {"MDR_ROLLOUT_RESIDENT_HOUSES": "0"}
SHAPES = {"fused256": ("k_step_fused<4,1,256>", 1024, 8), "fused128": ("k_step_fused<4,1,128>", 260, 3), "group32": ("k_step_group<32,1>", 20, 64)}
ENTRY_STEPS = (2, 3, 9, 19)
LOCK_STEPS = (2, 3, 6)
ENTRY_ITEMS = [("fused256", s) for s in SOURCES] + [(shape, s) for shape in ("fused128", "group32") for s in ("bangbang", "external")]
LOCK_ITEMS = [(shape, lockouts) for shape in sorted(SHAPES) for lockouts in ("column", "uniform")]
OK = "lean child ok: "


def _make(shape, seed):
    from tests.test_gpu_plan_oracle import _cfg, _env
    form, N, E = SHAPES[shape]
    assert pu.step_kernel(N, E) == form, (form, N, E, pu.step_kernel(N, E))
    env = _env(_cfg(N, 3), E, seed, TABLE_STEPS)
    env.reset(episode=1)
    assert env.rollout_resident(), shape
    return env, N, E


def _house_index(env):
    import torch
    E, N = env.t["sso"].shape
    return torch.arange(E, device="cuda:0").view(E, 1) * 5 + torch.arange(N, device="cuda:0").view(1, N)      # the pattern shifts from env to env


def _hand_in(env, ref, sd):
    from tests.test_gpu_rollout_interior import _prefill
    for e in (env, ref):
        e.load_state_dict(sd)
        _prefill(e)


def _run_entry(shape, source):
    import torch
    env, N, E = _make(shape, 977)
    external = source == "external"
    env.set_controller("bangbang" if external else source)
    dt = int(env.spec.time_step)
    L = env.t["lockout"].clone()
    assert int(L.min()) != int(L.max()), "the lockout column is streamed"
    on_sso = (torch.ones_like(L), torch.full_like(L, dt), L - dt, L, L + dt)
    off_sso = (torch.zeros_like(L), L - 2 * dt, L - dt, L)
    patterns = [(1, s, lock) for s in on_sso for lock in (0, 2)] + [(0, s, lock) for s in off_sso for lock in (0, 2)]
    pick = _house_index(env) % len(patterns)
    for j, (on, sso, lock) in enumerate(patterns):
        m = pick == j
        env.t["sso"][m] = sso.clamp(min=0)[m].to(env.t["sso"].dtype)
        env.t["flags"][m] = on | lock
    broken = int(((env.t["flags"] & 1) != 0).logical_and(env.t["sso"] != 0).sum())      # houses that break the invariant on entry
    sd = env.state_dict()
    ref = copy.deepcopy(env)
    bad = []
    for K in ENTRY_STEPS:
        _hand_in(env, ref, sd)
        act = _actions(E, N, 31 * K) if external else None
        for t in range(K):
            ref.step(act) if external else ref.step_controller()
        env.rollout(K, act)
        torch.cuda.synchronize()
        _compare("%s %s entry K=%d" % (shape, source, K), env, ref, bad)
    return {"shape": shape, "source": source, "on_with_sso": broken}, bad


def _run_lock(shape, lockouts):
    import torch
    env, N, E = _make(shape, 311)
    env.set_controller("bangbang")
    dt = int(env.spec.time_step)
    if lockouts == "column":
        L = torch.tensor([0, dt, 2 * dt, 5 * dt], device="cuda:0")[_house_index(env) % 4]
    else:
        L = torch.full(env.t["lockout"].shape, 5 * dt, device="cuda:0")
    env.t["lockout"].copy_(L.to(env.t["lockout"].dtype))
    ref = copy.deepcopy(env)
    bad, switched = [], {}
    for K in LOCK_STEPS:
        for run in ("on", "off"):
            if run == "on":
                env.t["flags"].fill_(0)
                env.t["sso"].copy_((L - (K - 1) * dt).clamp(min=0).to(env.t["sso"].dtype))
                env.t["flags"][env.t["sso"] < env.t["lockout"]] = 2
                act = torch.ones((E, N), dtype=torch.uint8, device="cuda:0")
            else:
                env.t["flags"].fill_(1)
                env.t["sso"].fill_(0)
                act = torch.zeros((E, N), dtype=torch.uint8, device="cuda:0")
            sd = env.state_dict()
            _hand_in(env, ref, sd)
            before = (ref.t["flags"] & 1).clone()
            for t in range(K):
                if t == K - 1:      # what the last interior step switched, on the twin
                    switched["%s K=%d" % (run, K)] = int(((ref.t["flags"] & 1) != before).sum())
                before = (ref.t["flags"] & 1).clone()
                ref.step(act)
            env.rollout(K, act)
            torch.cuda.synchronize()
            label = "%s lockout %s, %s K=%d" % (shape, lockouts, run, K)
            _compare(label, env, ref, bad)
            env.step(act)      # a plain step behind the rollout
            ref.step(act)
            torch.cuda.synchronize()
            _compare(label + " and a step", env, ref, bad)
    return {"shape": shape, "lockouts": lockouts, "switched": switched, "houses": E * N}, bad


def _child():
    kind, shape, arg = sys.argv[1:4]
    report, bad = (_run_entry if kind == "entry" else _run_lock)(shape, arg)
    print("REPORT " + json.dumps(report))
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print(OK + " ".join(sys.argv[1:]))


@pytest.mark.parametrize("shape,source", ENTRY_ITEMS)
def test_entry_states_that_break_the_invariant(shape, source):
    (r,) = run_child(ENVIRONMENT, "entry", shape, source, script=__file__, ok=OK)
    assert r["on_with_sso"] > 0, r


@pytest.mark.parametrize("shape,lockouts", LOCK_ITEMS)
def test_lock_bit_of_the_last_interior_step(shape, lockouts):
    (r,) = run_child(ENVIRONMENT, "lock", shape, lockouts, script=__file__, ok=OK)
    s = r["switched"]
    assert s["off K=2"] == r["houses"], r      # every house goes off in the only - the last - interior step
    if lockouts == "uniform":
        assert all(s["on K=%d" % K] == r["houses"] for K in LOCK_STEPS), r      # every house comes on in exactly the last interior step
    else:
        assert all(s["on K=%d" % K] > 0 for K in LOCK_STEPS), r


if __name__ == "__main__":
    _child()
