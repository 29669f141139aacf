"""tests/actor_forms.py (the actor kernels' selection, restated) against the case table of tests/test_gpu_actor_forms.py and against
the instantiations compiled into libmdr_hip.so - no compute, so no GPU needed: a form the launch code reaches without a GPU case, a
compiled instantiation nothing reaches, or a reachable one that is not compiled fails here."""
import collections
import os
import shutil

import numpy as np
import pytest
import torch

import mdr_amd
from tests import actor_forms as af
from tests import actor_ref as ar
from tests import test_gpu_actor_forms as gpu_cases

# compiled k_actor_* instantiations that no launch path selects, each with its reason (none today)
UNREACHABLE = {}


def test_every_reachable_form_has_a_gpu_case():
    forms = af.reachable_forms()
    count = collections.Counter(c["form"] for c in gpu_cases.CASES)
    assert forms - set(count) == set(), "forms without a GPU case: %s" % sorted(forms - set(count))
    assert set(count) - forms == set(), "cases outside the reachable forms: %s" % sorted(set(count) - forms)
    assert len(forms) == 87 and sum(1 for f in forms if "observe" in f) == 74
    assert max(count.values()) == 1      # one case per form: dropping any case uncovers its form
    # each case selects the form it names (the observe cases recompute theirs when the table is built: pin a few by hand)
    for c in gpu_cases.CASES:
        if c["kind"] == "rows":
            assert af.select_rows(c["layout"], c["F"], *c["layers"], A=gpu_cases.GRID_AGENTS)[0] == c["form"], c
    assert af.select_observe(1, 100, 100, 64, 5, rows_out=True) == ("k_actor_observe16<7,true,false,false,0,false>", 16)
    assert af.select_observe(3, 100, 100, 50, 37, True, 10, 18, False, False) == ("k_actor_observe16<7,false,true,true,15,false>", 16)
    assert af.select_observe(1, 127, 127, 50, 37, True, 10, 23, True, True) == ("k_actor_observe16<8,true,true,false,16,true>", 12)
    assert af.select_observe(2, 127, 127, 64, 5, True, 10, 23, False, True) == ("k_actor_observe_bf16<8,true,false,true,false>", 6)
    # the wave-count back-off of both extended families is among the cases
    for fam, full in (("k_actor_observe16", af.WAVES16_EXT), ("k_actor_observe_bf16", af.WAVESB)):
        waves = {c["waves"] for c in gpu_cases.CASES if c["kind"] == "observe" and af.family(c["form"]) == fam}
        assert full in waves and min(waves) < full, (fam, waves)
    # the on-rows batches fill the persistent grid more than once and end in a partial tile
    assert gpu_cases.GRID_AGENTS > 4 * 256 * 16 * 16 and gpu_cases.GRID_AGENTS % 16 != 0
    assert all(f in forms for f in (c["form"] for c in gpu_cases.FAMILY_CASES))
    assert {af.family(c["form"]) for c in gpu_cases.FAMILY_CASES} == {af.family(f) for f in forms}


def test_refusals_are_restated():
    assert af.select_rows(1, 129, 100, 100) == af.UNSUPPORTED and af.select_rows(0, 129, 100, 100)[0] == "k_actor_sample<0,0>"
    assert af.select_rows(3, 51, 100, 101) == af.UNSUPPORTED and af.select_rows(0, 51, 128, 100) == af.UNSUPPORTED
    assert af.select_rows(0, 51, 100, 100, feature_order=1) == af.INVALID and af.select_rows(0, 51, 100, 100, A=8, plane_stride=7) == af.INVALID
    assert af.select_rows(0, 250, 100, 100) == af.UNSUPPORTED                       # the fragments outgrow the LDS
    assert af.select_observe(0, 100, 100, 64) == af.UNSUPPORTED                     # the 32-agent layout has no observe -> act form
    assert af.select_observe(1, 100, 100, 10) == af.UNSUPPORTED                     # 10 houses have no 10 distinct neighbours
    assert af.select_observe(1, 100, 100, 64, ext=True, c=14, own=11) == af.UNSUPPORTED
    assert af.select_observe(1, 100, 100, 64, ext=True, c=13, own=13) == af.UNSUPPORTED      # 65 features
    assert af.select_observe(1, 100, 100, 64, num_state=47) == af.UNSUPPORTED and af.select_observe(1, 100, 100, 64, feature_order=0) == af.UNSUPPORTED
    assert af.rows_slices(128, gpu_cases.SLICE_AGENTS) == [(0, 8388592), (8388592, 5000)]
    assert af.rows_slices(51, 1000) == [(0, 1000)] and af.rows_slices(128, 9000000, plane_stride=9000000) == [(0, 9000000)]


def _readelf():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf"), os.path.join(rocm, "llvm", "bin", "llvm-readelf"),
                 "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/llvm/bin/llvm-readelf", shutil.which("llvm-readelf")):
        if cand and os.path.isfile(cand):
            return cand
    pytest.fail("llvm-readelf of the ROCm toolchain not found")


def test_compiled_instantiations_are_the_reachable_forms():
    """The kernel handles in the host image of libmdr_hip.so carry the mangled instantiation names; llvm-readelf --demangle of the
    toolchain that built them prints them (the ROCm tree ships no llvm-cxxfilt)."""
    library = mdr_amd.build_native()
    compiled = af.compiled_forms(library, _readelf())
    reachable = af.reachable_forms()
    assert len(compiled) >= 87
    stray = compiled - reachable - set(UNREACHABLE)
    assert stray == set(), "compiled but neither reachable nor listed as unreachable: %s" % sorted(stray)
    assert reachable - compiled == set(), "reachable but not compiled: %s" % sorted(reachable - compiled)
    assert set(UNREACHABLE) & reachable == set() and set(UNREACHABLE) <= compiled


def _judge_inputs(actor, rows, layout):
    """(torch fp32 forward / fp32 contract against fp64, share of agents whose logit difference lies inside the bound)."""
    with torch.no_grad():
        ref = actor(rows).numpy()
    d, p0, p1, bound = ar.forward64(*ar.module_weights(actor), rows.numpy(), layout=layout)
    ratio = float(np.maximum(ar.contract_ratio(ref[:, 0], p0, False), ar.contract_ratio(ref[:, 1], p1, False)).max())
    return ratio, float((np.abs(d) <= bound + 8 * ar.ulp32(d)).mean())


def test_gpu_case_inputs_keep_the_fp32_reference_inside_the_contract():
    """The inputs of the GPU cases, judged without a kernel: a torch fp32 forward of the same module against the fp64 one stays
    well inside the fp32 contract (so a kernel that exceeds it is wrong, not unlucky), and on the sparse networks no more than 1 %
    of the agents have a logit difference inside the derived bound of their layout (the greedy check's cap).  On-rows cases: their
    own rows (20,000 of them); observe -> act cases: the oracle's normStateDict rows of the same config, seed and episode after
    the same seven random steps (the device's rows to rounding)."""
    from oracle import mdr_oracle as mo
    from tests.test_gpu_observe_act import _shape_cfg
    worst = {"dense": 0.0, "sparse": 0.0}
    unclear = {"dense": 0.0, "sparse": 0.0}
    observe_rows = {}
    for c in gpu_cases.CASES:
        if c["kind"] == "rows":
            F, scale, seed = c["F"], gpu_cases.ROWS_SCALE, c["F"]
            rows = ar.rows_inputs(F, 20000, seed=20000)
        else:
            key = (c["N"], c["E"], c["extk"])
            if key not in observe_rows:
                shape = gpu_cases.SHAPES[c["extk"]]
                cfg = _shape_cfg(c["N"], shape["flags"], 10, shape["defects"])
                ora = mo.OracleEnv(cfg, nb_envs=c["E"]).reset(seed=5 + c["N"], episode=1)
                g = torch.Generator(device="cpu").manual_seed(c["extk"])      # the actions of tests/test_gpu_observe_act.py::_walk
                for _ in range(7):
                    ora.step((torch.rand((c["E"], c["N"]), generator=g) < 0.5).to(torch.uint8).numpy())
                ns = ora.norm_state(cfg)
                observe_rows[key] = torch.from_numpy(ns.reshape(c["E"] * c["N"], ns.shape[-1]).astype(np.float32))
            rows = observe_rows[key]
            F, scale, seed = rows.shape[1], gpu_cases.OBSERVE_SCALE, c["E"] + rows.shape[1]
        for net, keep, cap in gpu_cases.NETWORKS:
            ratio, share = _judge_inputs(ar.make_actor(F, c["layers"], seed, scale, keep), rows, c["layout"])
            worst[net], unclear[net] = max(worst[net], ratio), max(unclear[net], share)
            if cap:
                assert share <= 0.01, (c["form"], net, share)
    print("worst torch fp32 forward / fp32 contract %r, worst share inside the bound %r" % (worst, unclear))
    assert max(worst.values()) < 0.5
