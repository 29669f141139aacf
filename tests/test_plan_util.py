"""tests/plan_util.py against the library's own planner: mdr::plan_step / mdr::plan_rollout (exported from libmdr_hip.so, called
through ctypes on their mangled names - no compute, so no GPU needed), and the oracle case list of tests/test_gpu_plan_oracle.py
against reachable_forms(): a planner branch without an oracle case fails here."""
import ctypes as C
import os

import pytest

import mdr_amd
from tests import plan_util as pu

PLAN_KNOBS = ("MDR_PLAN_MULTI", "MDR_PLAN_PACKED", "MDR_PLAN_PACKED_FILL", "MDR_PLAN_THREADS", "MDR_SPLIT_THREADS")

EDGE_N = [255, 256, 257, 508, 512, 513, 1020, 1024, 1028, 2048, 2052, 4096, 4100]
GRID_E = [1, 2, 3, 37, 4096, 65535, 262144, 262145]


class StepPlan(C.Structure):      # mdr_kernels.h:222
    _fields_ = [("kind", C.c_int), ("vec", C.c_int), ("threads", C.c_int), ("tiles", C.c_int)]


@pytest.fixture(scope="module")
def planner():
    set_knobs = [k for k in PLAN_KNOBS if k in os.environ]
    if set_knobs:
        pytest.fail("planner knobs set in the environment: %s (the restatement assumes them unset)" % set_knobs)
    mdr_amd.build_native()
    lib = mdr_amd.load_native()
    fns = {}
    for name, sym in (("step", "_ZN3mdr9plan_stepEil"), ("rollout", "_ZN3mdr12plan_rolloutEil")):
        f = getattr(lib, sym)
        f.argtypes = [C.c_int, C.c_int64]
        f.restype = StepPlan
        fns[name] = f
    return fns


def _grid():
    for N in list(range(1, 161)) + EDGE_N:
        es = set(GRID_E)
        e0 = -(-pu.DEVICE_FILL // N)
        es.update((e0 - 1, e0))             # E * N just below and at / just above 262144
        if e0 * N == pu.DEVICE_FILL:
            es.add(e0 + 1)
        for E in sorted(e for e in es if e >= 1):
            yield N, E


def test_restatement_matches_the_library_planner(planner):
    bad = []
    n = 0
    for N, E in _grid():
        for name, ref in (("step", pu.plan_step), ("rollout", pu.plan_rollout)):
            p = planner[name](N, E)
            got = (p.kind, p.vec, p.threads, p.tiles)
            want = ref(N, E)
            n += 1
            if got != want:
                bad.append((name, N, E, got, want))
    assert n > 3000
    assert not bad, "%d of %d plans differ, first: %s" % (len(bad), n, bad[:5])


def test_grid_crosses_the_device_filling_edge():
    assert any(N * E == pu.DEVICE_FILL - 1 or (N * E < pu.DEVICE_FILL and N * (E + 1) >= pu.DEVICE_FILL) for N, E in _grid())
    assert any(N * E >= pu.DEVICE_FILL and N * (E - 1) < pu.DEVICE_FILL for N, E in _grid())


def test_every_reachable_form_has_an_oracle_case_and_no_case_strays():
    forms = pu.reachable_forms()
    cases = pu.oracle_cases()
    covered = {c[0] for c in cases}
    assert forms - covered == set(), "forms without an oracle case: %s" % sorted(forms - covered)
    assert covered - forms == set(), "cases outside the reachable forms: %s" % sorted(covered - forms)
    for form, N, E, ctl in cases:
        assert 1 <= N <= pu.MAX_N and E >= 1
        assert pu.case_forms(N, E, ctl) == form, (form, N, E, ctl)
    # the device-filling forms the small-batch suites never reach are in the set
    for form in ("k_step_group<16,4>", "k_step_group<8,4>", "k_step_group<1,4>", "k_step_single_house", "k_step_packed",
                 "k_step_multi<32>", "k_rollout_group<1,1,false,true>", "k_rollout_group<1,1,false,false>",
                 "k_rollout_group<8,4,false,false>", "k_rollout_fused<4,1,64,false,false>", "k_rollout_fused<4,2,256,false,false>",
                 "k_rollout_packed<false>"):
        assert form in forms, form


def test_case_batches_are_odd_where_the_form_allows():
    for form, N, E, ctl in pu.oracle_cases():
        if E % 2 == 0:          # even only where E + 1 selects another form (k_step_single_house: E % 4 == 0)
            assert pu.case_forms(N, E + 1, ctl) != form, (form, N, E)


def test_forms_restate_the_launch_switches():
    assert pu.step_kernel(1024, 4096) == "k_step_fused<4,1,256>"               # the benchmark's batch
    assert pu.rollout_kernel(1024, 4096, "bangbang") == "k_rollout_fused<4,1,256,false,true>"
    assert pu.step_kernel(50, 5243) == "k_step_multi<32>" and pu.rollout_kernel(50, 5243, "deadband") == "k_rollout_group<32,2,false,false>"
    assert pu.step_kernel(1, 262144) == "k_step_single_house" and pu.rollout_kernel(1, 262144) == "k_rollout_group<1,1,false,true>"
    assert pu.step_kernel(1, 262145) == "k_step_group<1,1>"
    assert pu.step_kernel(36, 7281) == "k_step_group<64,1>" and pu.step_kernel(36, 7283) == "k_step_packed"
    assert pu.step_kernel(1025, 3) == "k_step_partial<1,256>+k_step_finish<1,256>" and pu.rollout_kernel(1025, 3) is None
    assert pu.rollout_kernel(516, 254, "always_on") == "k_rollout_fused<4,1,256,true,false>"
    assert pu.rollout_kernel(516, 512, "always_on") == "k_rollout_fused<4,1,256,false,false>"
    assert pu.rocprof_name("k_rollout_group<8,4,false,true>") == "mdr::k_rollout_group<8, 4, false, true>"
