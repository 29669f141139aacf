"""Differential fuzz of rollout() on the resident arm: the seeded cases 0 .. 87 of tests/test_gpu_fuzz_rollout.py (draw: every EDGE_N
twice, dt of 1 to 60 s, tables of 3, 8 and 64 rows, every signal family, deadband 0, lockout 0 houses, noise-free houses, every
N % 4; per case 0 .. 4 warm-up single steps, K in 1 .. 40, its own action source) with MDR_ROLLOUT_RESIDENT_HOUSES=0, so that
every case whose step form has an interior instantiation runs k_rollout_resident / k_rollout_resident_group - from wherever in the
tables the warm-up left the cursor, over as many refills as K asks for.

rollout(K) must leave what K single steps on a deep copy leave, bit for bit (NaNs as bits) over Ta, Tm, sso, flags, actions, reward,
P and the seven obs planes, every output sentinel-filled before the call; and the twin's steps go through the fp64 oracle on the whole
batch, as tests/test_gpu_fuzz_rollout.py does for its `stream` plan (the run is that file's _run_case under that plan's knobs: no
local plane, the thermal pack read by the resident launches, the records held to the numpy reference).

Every item asserts from what its child reports that each fused / group case of its chunk reported rollout_resident() True and every
other case False (read in the child from a handle built as the case's: the switch depends on the process's knobs and the handle's
shape and mode alone); tests/test_rollout_fuzz_cases.py's census says 76 of the 88, recounted here.  (A case with K = 1 is the full last
step alone: the switch says resident, and no interior step exists to run.)"""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_fuzz_rollout as fr      # noqa: E402
from tests.test_gpu_rollout_forms import PLANS, FULL_STEPS, child_main      # noqa: E402
from tests.test_gpu_rollout_resident import run_child      # noqa: E402

ENVIRONMENT = dict(PLANS["stream"][0], MDR_ROLLOUT_RESIDENT_HOUSES="0")
NB_CHUNKS = -(-fr.BASE_CASES // fr.CHUNK)


def _chunk(arg):
    lo = int(arg) * fr.CHUNK
    return list(range(lo, min(lo + fr.CHUNK, fr.BASE_CASES)))


def _run_case(plan, idx):
    import mdr_amd
    report, bad = fr._run_case(plan, idx)
    # the switch depends on the process's knobs and the handle's shape and mode: a handle built as the case's says what its rollout() took
    cfg, E, N, seed, episode, _, table_steps = fr.draw(idx)[:7]
    probe = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=table_steps)
    probe.reset(episode=episode)
    report["resident"] = probe.rollout_resident()
    return report, bad


def interior_cases():
    return [idx for idx in range(fr.BASE_CASES) if fr.takes_interior(fr.draw(idx)[2], fr.draw(idx)[1])]


@pytest.mark.parametrize("chunk", range(NB_CHUNKS))
def test_fuzz_resident_rollout_equals_single_steps(chunk):
    reports = run_child(ENVIRONMENT, "stream", chunk, script=__file__, ok="rollout child ok: ")
    assert [r["idx"] for r in reports] == _chunk(chunk)
    for r in reports:
        interior = fr.takes_interior(r["N"], r["E"])
        assert r["resident"] == interior, r
        assert (r["planes"], r["packed"]) == (PLANS["stream"][1] if interior else FULL_STEPS), r      # the plan keeps its answers
        assert r["ref_packed"] and (not interior or r["desc"] == 1), r
    assert sum(r["resident"] for r in reports) == len([i for i in interior_cases() if i in _chunk(chunk)])
    assert len(interior_cases()) == 76      # the CPU census of tests/test_rollout_fuzz_cases.py, recounted


if __name__ == "__main__":
    child_main(_run_case, _chunk)
