"""What the cases of the rollout() tests are, recomputed without a GPU from the planner's restatement (tests/plan_util.py), the
oracle's reset and the numpy pack reference: the conditions tests/test_gpu_rollout_forms.py and tests/test_gpu_fuzz_rollout.py rely
on to reach the interior forms and the PACK decode.  If the case sets change, the numbers here say what they stopped covering."""
import pytest

from oracle import mdr_oracle as mo
from tests import plan_util as pu
from tests import thermal_pack_ref as tp
from tests.test_gpu_fuzz_rollout import BASE_CASES, CHUNK, NB_CHUNKS, SOURCES, _chunk, base_interior_cases, draw, takes_interior
from tests.test_gpu_rollout_forms import CASES, CHUNKS, PLANS, has_interior
from tests.test_gpu_rollout_forms import _chunk as forms_chunk


def test_form_cases_are_the_33_step_forms():
    forms = [c[0] for _, c in CASES]
    assert sorted(forms) == sorted(f for f in pu.reachable_forms() if f.startswith("k_step_")) and len(forms) == 33
    assert [c for _, c in CASES] == [c for c in pu.oracle_cases() if c[3] is None]
    assert sum(has_interior(f) for f in forms) == 25
    assert sorted(f for f in forms if not has_interior(f)) == [
        "k_step_multi<16>", "k_step_multi<32>", "k_step_multi<4>", "k_step_multi<64>", "k_step_multi<8>", "k_step_packed",
        "k_step_partial<1,256>+k_step_finish<1,256>", "k_step_single_house"]
    for _, (form, N, E, _) in CASES:
        assert pu.step_kernel(N, E) == form
        assert E % 2 == 1 or pu.step_kernel(N, E + 1) != form      # odd where possible: a part-filled last wave
    assert sorted(ic for c in range(CHUNKS) for ic in forms_chunk(c)) == sorted(CASES)
    assert max(N * E for _, (_, N, E, _) in CASES) == 262208
    assert sorted(PLANS) == ["default", "planes5", "stream", "stream_nopack"]
    # below the default threshold of MDR_ROLLOUT_STREAM_HOUSES (1 << 20 houses): the unset plan keeps its two local planes
    assert all(N * E < 1 << 20 for _, (_, N, E, _) in CASES)


@pytest.fixture(scope="module")
def census():
    rows = []
    for idx in range(BASE_CASES):
        cfg, E, N, seed, episode, _, table_steps, pre, K, source = draw(idx)
        ora = mo.OracleEnv(cfg, nb_envs=E).reset(seed=seed, episode=episode)
        cols = tp.thermal_columns(ora.Ua, ora.Cm, ora.Ca, ora.Hm, ora.spec.dt)
        rows.append(dict(idx=idx, N=N, E=E, kind=pu.plan_step(N, E)[0], packed=tp.describe(cols)[0], widths=tp.needed_widths(cols),
                         lockout0=bool((ora.lockout == 0).any()), dt=int(ora.spec.dt), table_steps=table_steps, pre=pre, K=K,
                         source=source, deadband=float(ora.spec.deadband)))
    return rows


def test_fuzz_cases_reach_the_interior_forms_and_the_pack(census):
    assert len(census) == BASE_CASES == 88 and NB_CHUNKS * CHUNK >= BASE_CASES
    assert sorted(i for c in range(-(-BASE_CASES // CHUNK)) for i in _chunk(c) if i < BASE_CASES) == list(range(BASE_CASES))
    assert all(r["N"] * r["E"] <= 20000 for r in census)                       # the oracle runs on the whole batch
    interior = [r for r in census if r["kind"] in (pu.STEP_FUSED, pu.STEP_GROUP)]
    assert len(interior) == base_interior_cases() == 76                        # these take an interior plan
    assert all(takes_interior(r["N"], r["E"]) == (r in interior) for r in census)
    assert sum(r["kind"] == pu.STEP_SPLIT for r in census) == 12               # these take rollout_split
    assert all(r["packed"] for r in census)                                    # the reference packs every one
    single = [r for r in census if r["widths"] == (0, 0, 0, 0, 0)]             # noise-free houses: five zero fields, the base carries the value
    assert len(single) == 35
    wide = [r for r in census if r not in single]
    assert len(wide) == 53 and all(19 <= w <= 26 for r in wide for w in r["widths"])
    assert all(w <= have for r in wide for w, have in zip(r["widths"], tp.WIDTHS))
    lockout0 = [r for r in census if r["lockout0"]]                            # houses with lockout == 0: a 0/0 plane 4
    assert len(lockout0) == 11 and sum(r in interior for r in lockout0) == 9


def test_fuzz_cases_cover_the_configuration_space(census):
    assert {r["N"] % 4 for r in census} == {0, 1, 2, 3}
    assert {r["dt"] for r in census} == {1, 4, 7, 30, 60}
    assert {r["table_steps"] for r in census} == {3, 8, 64}
    assert {r["source"] for r in census} == set(SOURCES)
    assert {r["pre"] for r in census} == {0, 1, 2, 3, 4}
    assert min(r["K"] for r in census) >= 1 and max(r["K"] for r in census) <= 40
    assert any(r["K"] > r["table_steps"] for r in census if r["kind"] in (pu.STEP_FUSED, pu.STEP_GROUP))      # refills inside a rollout
    assert any(r["deadband"] == 0 and r["source"] == "deadband" for r in census)
