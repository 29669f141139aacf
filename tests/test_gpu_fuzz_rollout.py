"""Differential fuzz of rollout(): the seeded (shape, config) cases of tests/test_gpu_fuzz.py (_case: every EDGE_N twice, dt of 1 to
60 s, tables of 3, 8 and 64 rows, every signal family, random penalty weights, deadband 0, lockout 0 houses with their 0/0 plane 4,
noise-free houses whose thermal columns hold one value, every N % 4) under each of the four interior plans of
tests/test_gpu_rollout_forms.py.

Per case, from an rng of its own: 0 .. 4 warm-up single steps, K in 1 .. 40, the action source (bang-bang twice as likely, deadband,
always-on, external).  rollout(K) must leave what K single steps on a deep copy leave, bit for bit (NaNs as bits) over Ta, Tm, sso,
flags, actions, reward, P and the seven obs planes, every output sentinel-filled before the call.

Under `stream` (the benchmark's plan: no local plane, the PACK decode) the twin's steps also go through the fp64 oracle on the whole
batch (E * N <= 20,000): it replays the twin's recorded actions, a controller may decide otherwise than the oracle's rule only
within EDGE_RTOL of a threshold, and the end state is held to the tolerances of test_fuzz_device_vs_oracle; and the records and the
descriptor on the device are held to the numpy reference.

tests/test_rollout_fuzz_cases.py pins, without a GPU, what the first 88 cases are: 76 select a fused or group form and so an interior
plan, 12 the split path, all 88 are packed by the reference.  Here every item asserts from what its child reports that each fused /
group case of its chunk ran with planes >= 0 - and under `stream` with the pack in the plan and a descriptor word of 1 - so over the
chunks at least 76 cases reach the interior forms and the PACK decode; a case set that stops reaching them fails instead of
passing on nothing.  MDR_FUZZ_SCALE=k runs 88 * k cases, as in tests/test_gpu_fuzz.py."""
import copy
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import plan_util as pu      # noqa: E402
from tests.test_gpu_fuzz import SCALE, _case      # noqa: E402
from tests.test_gpu_rollout_forms import FULL_STEPS, PLANS, child_main, run_child, same_bits      # noqa: E402

BASE_CASES = 88                      # every EDGE_N twice
CHUNK = 44                           # cases per child
SOURCES = ("bangbang", "bangbang", "deadband", "always_on", "external")
INTERIOR_KINDS = (pu.STEP_FUSED, pu.STEP_GROUP)


def draw(idx):
    """The case: tests/test_gpu_fuzz.py's (cfg, E, N, seed, episode, p_on, table_steps) and, from a stream of its own (the cases of
    the files before stay what they are), the warm-up steps, K and the action source."""
    cfg, E, N, seed, episode, p_on, table_steps = _case(idx)
    rng = np.random.default_rng(31000 + idx)
    pre, K, source = int(rng.integers(0, 5)), int(rng.integers(1, 41)), SOURCES[int(rng.integers(0, len(SOURCES)))]
    return cfg, E, N, seed, episode, p_on, table_steps, pre, K, source


def takes_interior(N, E):
    return pu.plan_step(N, E)[0] in INTERIOR_KINDS


def _run_case(plan, idx):
    import torch
    import mdr_amd
    from mdr_amd import _native as nat
    from tests import thermal_pack_ref as tp
    from tests.slice_oracle import SliceOracle
    from tests.test_gpu_rollout_interior import COMPARED, _prefill
    from tests.test_gpu_thermal_pack import _device_pack, _pack_matches
    cfg, E, N, seed, episode, p_on, table_steps, pre, K, source = draw(idx)
    external = source == "external"
    label = "fuzz case %d (N=%d E=%d %s, %s, pre=%d K=%d, tables of %d), plan %s" % (idx, N, E, pu.step_kernel(N, E), source, pre, K, table_steps, plan)
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=table_steps)
    env.reset(episode=episode)
    env.set_controller("bangbang" if external else source)
    bad = []
    want = PLANS[plan][1] if takes_interior(N, E) else FULL_STEPS
    got = env.rollout_plan()
    if got != want:
        bad.append("%s: plan %s, expected %s" % (label, got, want))
    act = None
    if external:
        act = (torch.rand((E, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(idx)) < p_on).to(torch.uint8)
    # the whole batch in one slice: SliceOracle's oracle is OracleEnv(cfg, nb_envs=E).reset(seed, episode)
    sl = SliceOracle(cfg, env, seed, episode, k=E, offsets=[0]) if plan == "stream" else None
    last_reward = [None]

    def single(e, where):
        """One single step on `e`; with the oracle: the decisions against its rule, and it replays the recorded actions."""
        want_act = None if sl is None or external else sl.decisions(source)
        e.step(act) if external else e.step_controller()
        if sl is None:
            return
        acts = sl.take(act if external else e.t["actions"])
        if not external:
            diff, off_edge = sl.decision_misses(acts, source, want_act)
            assert off_edge == 0, "%s: %d %s decisions differ away from a threshold" % (where, off_edge, source)
        sl.step(acts)
        last_reward[0] = sl.rewards[0]

    for t in range(pre):
        single(env, "%s, warm-up step %d" % (label, t))
    ref = copy.deepcopy(env)
    _prefill(env)
    _prefill(ref)
    for t in range(K):
        single(ref, "%s, single step %d" % (label, t))
    env.rollout(K, act)
    torch.cuda.synchronize()
    assert env.steps_taken == ref.steps_taken == pre + K, (label, env.steps_taken, ref.steps_taken)
    for k in COMPARED:
        if not same_bits(env.t[k], ref.t[k]):
            differ = int((env.t[k].contiguous().view(torch.uint8) != ref.t[k].contiguous().view(torch.uint8)).sum())
            bad.append("%s %s: %d of %d bytes differ" % (label, k, differ, env.t[k].numel() * env.t[k].element_size()))
    desc_word = expect = None
    if sl is not None:
        # the end state under the tolerances of tests/test_gpu_fuzz.py::test_fuzz_device_vs_oracle (its reward scale and atol)
        ora = sl.oras[0]
        rw = cfg["default_env_prop"]["reward_prop"]
        scale = max(1.0, float(rw["alpha_temp"]) + float(rw["alpha_sig"]))
        flags = ref.t["flags"].cpu().numpy()
        np.testing.assert_array_equal((flags & 1).astype(bool), ora.on, err_msg=label)
        np.testing.assert_array_equal((flags & 2).astype(bool), ora.lock, err_msg=label)
        np.testing.assert_array_equal(ref.t["sso"].cpu().numpy(), ora.sso, err_msg=label)
        np.testing.assert_allclose(ref.t["P"].cpu().numpy(), ora.P, rtol=1e-12, err_msg=label)
        np.testing.assert_allclose(ref.house_temp().cpu().numpy(), ora.Ta, rtol=1e-5, err_msg=label)
        np.testing.assert_allclose(ref.house_mass_temp().cpu().numpy(), ora.Tm, rtol=1e-5, err_msg=label)
        np.testing.assert_allclose(ref.reg_signal().cpu().numpy(), ora.S, rtol=1e-9, atol=1e-6, err_msg=label)
        np.testing.assert_allclose(ref.t["reward"].cpu().numpy(), last_reward[0], rtol=1e-5, atol=1e-5 * scale, err_msg=label)
        np.testing.assert_allclose(ref.obs_vector("rows").cpu().numpy(), ora.norm_state(cfg), rtol=3e-5, atol=3e-6, err_msg=label)
        # the first 88 cases are packed by the reference (tests/test_rollout_fuzz_cases.py); beyond them, whatever the reference says
        expect = True if idx < BASE_CASES else bool(tp.describe([env.t[c].cpu().numpy() for c in tp.COLUMNS])[0])
        bad += _pack_matches(label, env, expect_packed=expect)
        desc_word = int(_device_pack(env)[0][nat.MDR_THERMAL_DESC_PACKED])
    return {"idx": idx, "N": N, "E": E, "planes": got[0], "packed": bool(got[1]), "desc": desc_word, "ref_packed": expect}, bad


def _chunk(arg):
    lo = int(arg) * CHUNK
    return list(range(lo, min(lo + CHUNK, BASE_CASES * SCALE)))


NB_CHUNKS = -(-BASE_CASES * SCALE // CHUNK)


@functools.lru_cache(maxsize=None)
def base_interior_cases():
    """How many of the first 88 cases select a fused or group form (tests/test_rollout_fuzz_cases.py pins it: 76)."""
    return sum(takes_interior(c[2], c[1]) for c in (draw(idx) for idx in range(BASE_CASES)))


@pytest.mark.parametrize("chunk", range(NB_CHUNKS))
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_fuzz_rollout_equals_single_steps(plan, chunk):
    reports = run_child(__file__, plan, chunk)
    assert [r["idx"] for r in reports] == _chunk(chunk)
    interior = [r for r in reports if takes_interior(r["N"], r["E"])]
    for r in reports:
        want = PLANS[plan][1] if takes_interior(r["N"], r["E"]) else FULL_STEPS
        assert (r["planes"], r["packed"]) == want, r
    assert sum(r["planes"] >= 0 for r in reports) == len(interior)
    if plan == "stream":
        assert all(r["ref_packed"] for r in reports if r["idx"] < BASE_CASES)
        assert sum(r["packed"] and r["desc"] == int(r["ref_packed"]) for r in interior) == len(interior)
    # over idx 0 .. 87 at least 76 cases take an interior plan (under `stream`: the PACK decode, descriptor word 1), and each chunk
    # has just shown that all of its own did
    assert base_interior_cases() >= 76


if __name__ == "__main__":
    child_main(_run_case, _chunk)
