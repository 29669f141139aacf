"""The thermal pack on the device (mdr_env_bind_thermal_pack) and the size rule of mdr_env_rollout's interior steps.

With MDR_ROLLOUT_STREAM_HOUSES=0 every batch is a "large" one: the interior steps store no local obs plane and run the PACK form of
k_step_fused / k_step_group.  After reset the records and the descriptor on the device must equal the numpy reference
(tests/thermal_pack_ref.py) bit for bit, and rollout(K) must leave what K single steps leave, bit for bit, over Ta, Tm, sso, flags,
reward, obs, actions and P - K = 70 crosses a refill of the 64-row tables.  Also: the fallback when a column cannot be packed, the
two switches, the unset threshold (the parent's plan at these sizes, read from mdr_env_rollout_plan, not from a clock), a
snapshot taken without a pack loaded into an env with one, and the field boundaries: a column whose range fills its field exactly
(an all-ones field, through load_thermal's masks) and one a single pattern wider (k_thermal_range's "not packed").

The knobs are read once per process: every test starts one fresh child (this file run as a script, never an exec) under its own
timeout."""
import copy
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_COUNTS = (1, 2, 5, 70)
TABLE_STEPS = 64
# (E, N): the form the step planner picks for it (tests/plan_util.py) - the smallest shapes that reach a different path each
SHAPES = {(2, 1024): "k_step_fused<4,1,256>",     # the benchmark's form
          (2, 2048): "k_step_fused<4,2,256>",     # two tiles
          (3, 1000): "k_step_fused<4,1,256>",     # a partly empty last wave
          (5, 20): "k_step_group<32,1>", (5, 50): "k_step_group<64,1>", (7, 6): "k_step_group<8,1>",     # small batches run one house per lane
          (3, 68): "k_step_group<32,4>", (3, 66): "k_step_group<64,2>",                                    # 16- and 8-byte record loads, idle lanes
          (3, 65): "k_step_fused<1,1,256>"}       # 4-byte record loads in the fused form
CHILD_TIMEOUT = 300
KNOBS = ("MDR_ROLLOUT_INTERIOR", "MDR_ROLLOUT_INTERIOR_PLANES", "MDR_ROLLOUT_STREAM_HOUSES", "MDR_THERMAL_PACK")


def _make(cfg, E, controller="bangbang", **kw):
    import mdr_amd
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=7, table_steps=TABLE_STEPS, **kw)
    env.set_controller(controller)
    return env


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.numel() else a.numel() == b.numel()


def _rollout_matches(label, env, external=False, counts=STEP_COUNTS, reset=True):
    """rollout(K) on `env` against K single steps on a deep copy of it; the list of mismatches."""
    import torch
    from tests.test_gpu_rollout_interior import COMPARED, _prefill
    E, N = env.nb_envs, env.nb_houses
    bad = []
    for K in counts:
        if reset:
            env.reset(episode=0)
        ref = copy.deepcopy(env)
        _prefill(env)
        _prefill(ref)
        act = None
        if external:
            act = (torch.rand((E, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(K)) < 0.6).to(torch.uint8)
        for _ in range(K):
            ref.step(act) if external else ref.step_controller()
        env.rollout(K, act)
        torch.cuda.synchronize()
        assert env.steps_taken == ref.steps_taken
        for k in COMPARED:
            if not _same_bits(env.t[k], ref.t[k]):
                bad.append("%s K=%d %s: %d of %d elements differ" % (label, K, k, int((env.t[k] != ref.t[k]).sum()), env.t[k].numel()))
    return bad


def _device_pack(env):
    import numpy as np
    import torch
    torch.cuda.synchronize()
    desc = env.t["thermal_desc"].cpu().numpy().view(np.uint32)
    planes = env.t["thermal_pack"].cpu().numpy().view(np.uint32).reshape(4, -1)
    return desc, planes


def _pack_matches(label, env, expect_packed=True):
    """The descriptor and the records on the device against the numpy reference on the device's own five columns."""
    import numpy as np
    from mdr_amd import _native as nat
    from tests import thermal_pack_ref as tp
    desc, planes = _device_pack(env)
    packed, bases, ref = tp.pack([env.t[c].cpu().numpy() for c in tp.COLUMNS])
    bad = []
    if packed != expect_packed or int(desc[nat.MDR_THERMAL_DESC_PACKED]) != int(expect_packed):
        bad.append("%s: packed %d on the device, %d in the reference, expected %d" % (label, desc[0], packed, expect_packed))
    if not np.array_equal(desc[nat.MDR_THERMAL_DESC_BASE:nat.MDR_THERMAL_DESC_BASE + 5], bases):
        bad.append("%s: bases differ" % label)
    if packed and not np.array_equal(planes, ref):
        bad.append("%s: %d of %d record words differ" % (label, int((planes != ref).sum()), ref.size))
    return bad


def _shapes(controller, external, plan, pack_check):
    from tests import plan_util as pu
    from tests.test_gpu_rollout_interior import _cfg
    bad = []
    for (E, N), form in SHAPES.items():
        assert pu.step_kernel(N, E) == form, ((E, N), pu.step_kernel(N, E), form)
        env = _make(_cfg(N), E, controller)
        label = "%dx%d %s %s" % (E, N, form, "external" if external else controller)
        if env.rollout_plan() != plan:
            bad.append("%s: plan %s, expected %s" % (label, env.rollout_plan(), plan))
        bad += _rollout_matches(label, env, external)
        if pack_check:
            bad += _pack_matches(label, env)
    return bad


def _mode_forms(arg):
    """MDR_ROLLOUT_STREAM_HOUSES=0: count 0 and the PACK form at every shape."""
    return _shapes("bangbang" if arg == "external" else arg, arg == "external", (0, True), True)


def _mode_pack_off(arg):
    """MDR_ROLLOUT_STREAM_HOUSES=0 and MDR_THERMAL_PACK=0: count 0, the five columns streamed - the same bits."""
    return _shapes("bangbang", False, (0, False), False)


def _mode_unset(arg):
    """No knob set: these shapes are below the threshold and take the parent's plan - two local planes, no pack."""
    return _shapes("bangbang", False, (2, False), True)      # (the records are built whether a launch reads them or not)


def _mode_extras(arg):
    """MDR_ROLLOUT_STREAM_HOUSES=0: the fallback, the constructor switch, a snapshot from an env without a pack."""
    import torch
    from tests.test_gpu_rollout_interior import _cfg
    bad = []
    for E, N in ((2, 1024), (5, 20)):
        env = _make(_cfg(N), E)
        env.reset(episode=0)
        bad += _pack_matches("%dx%d before" % (E, N), env)
        k01 = env.t["k01"]
        keep = k01[E - 1, N // 2].clone()
        k01[E - 1, N // 2] = -keep                       # both signs in one column: cannot be packed
        env.params_changed()
        bad += _pack_matches("%dx%d negated k01" % (E, N), env, expect_packed=False)
        if env.rollout_plan() != (0, True):              # the PACK form is still what runs: its streaming arm
            bad.append("%dx%d fallback: plan %s" % (E, N, env.rollout_plan()))
        bad += _rollout_matches("%dx%d fallback" % (E, N), env, reset=False, counts=(1, 5, 70))
        k01[E - 1, N // 2] = keep
        env.params_changed()
        bad += _pack_matches("%dx%d restored" % (E, N), env)
        bad += _rollout_matches("%dx%d restored" % (E, N), env, reset=False, counts=(2, 70))

        plain = _make(_cfg(N), E, thermal_pack=False)     # the constructor switch: nothing bound, count 0, the same bits
        if plain.rollout_plan() != (0, False) or "thermal_pack" in plain.t:
            bad.append("%dx%d thermal_pack=False: plan %s" % (E, N, plain.rollout_plan()))
        bad += _rollout_matches("%dx%d thermal_pack=False" % (E, N), plain)

        # a snapshot from an env without a pack - what a state_dict from before the pack existed holds - loads into an env with
        # one, and the records are rebuilt from the arrays it brought
        plain.reset(episode=3)
        plain.rollout(5)
        sd = plain.state_dict()
        assert sorted(sd) == ["episode", "j0", "k", "od_table", "seed", "slab"]
        env.reset(episode=0)
        env.load_state_dict(sd)
        if not _same_bits(env.t["k01"], plain.t["k01"]):
            bad.append("%dx%d snapshot: k01 not loaded" % (E, N))
        bad += _pack_matches("%dx%d snapshot" % (E, N), env)
        env.rollout(70)
        plain.rollout(70)
        torch.cuda.synchronize()
        for k in ("Ta", "Tm", "sso", "flags", "reward", "obs", "actions", "P"):
            if not _same_bits(env.t[k], plain.t[k]):
                bad.append("%dx%d snapshot, 70 steps on: %s differs" % (E, N, k))
    return bad


def _set_pattern(env, name, house, pattern):
    """Writes a u32 bit pattern into one house of a column, through an int32 view of the column."""
    import torch
    env.t[name].view(torch.int32).view(-1)[house] = pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def _all_ones_fields(label, env, tops):
    """{column index: house}: the house holding the column's largest pattern carries an all-ones field in the device's records."""
    from tests import thermal_pack_ref as tp
    got = tp.fields(_device_pack(env)[1])
    return ["%s: field %s of house %d is %#x, not all ones" % (label, tp.COLUMNS[c], h, int(got[c][h]))
            for c, h in tops.items() if int(got[c][h]) != (1 << tp.WIDTHS[c]) - 1]


def _mode_edges(arg):
    """MDR_ROLLOUT_STREAM_HOUSES=0: a field that is exactly full (max - min == 2^w - 1: packed, all ones in the records, the PACK
    decode's masks at the dword boundaries) and a range one pattern too wide (2^w: k_thermal_range must say not packed), per column
    and for all five columns at once; rollout(K) against single steps each time."""
    from tests import thermal_pack_ref as tp
    from tests.test_gpu_rollout_interior import _cfg
    bad = []
    for E, N in ((2, 1024), (5, 20)):
        env = _make(_cfg(N), E)
        env.reset(episode=0)
        bad += _pack_matches("%dx%d before" % (E, N), env)
        if env.rollout_plan() != (0, True):
            bad.append("%dx%d: plan %s" % (E, N, env.rollout_plan()))
        orig = {name: env.t[name].clone() for name in tp.COLUMNS}
        patterns = [tp.bits(orig[name].cpu().numpy()) for name in tp.COLUMNS]
        tops = {c: int(b.argmax()) for c, b in enumerate(patterns)}
        his = {c: int(b.max()) for c, b in enumerate(patterns)}
        houses = {}
        for c, (name, b) in enumerate(zip(tp.COLUMNS, patterns)):
            # a house of its own per column, never one that holds a column's largest pattern
            houses[c] = next(h for h in range(b.size) if h not in houses.values() and h not in tops.values())
            span = 1 << tp.WIDTHS[c]
            # hi - 2^w: the same sign, a smaller magnitude, still a normal number, and below the column's smallest pattern
            assert (his[c] & 0x7FFFFFFF) - span >= 0x00800000 and his[c] - span + 1 < int(b.min()), (name, hex(his[c]))
        for c, name in enumerate(tp.COLUMNS):
            w = tp.WIDTHS[c]
            label = "%dx%d %s" % (E, N, name)
            _set_pattern(env, name, houses[c], his[c] - ((1 << w) - 1))          # the field is exactly full
            env.params_changed()
            bad += _pack_matches(label + " range 2^%d - 1" % w, env)
            bad += _all_ones_fields(label + " range 2^%d - 1" % w, env, {c: tops[c]})
            bad += _rollout_matches(label + " range 2^%d - 1" % w, env, reset=False, counts=(2, 70))
            _set_pattern(env, name, houses[c], his[c] - (1 << w))                # one pattern too wide
            env.params_changed()
            bad += _pack_matches(label + " range 2^%d" % w, env, expect_packed=False)
            if env.rollout_plan() != (0, True):                                  # the PACK form still runs: its streaming arm
                bad.append("%s range 2^%d: plan %s" % (label, w, env.rollout_plan()))
            bad += _rollout_matches(label + " range 2^%d" % w, env, reset=False, counts=(2, 70))
            env.t[name].copy_(orig[name])
        for c, name in enumerate(tp.COLUMNS):                                    # all five at full width, a house per column
            _set_pattern(env, name, houses[c], his[c] - ((1 << tp.WIDTHS[c]) - 1))
        env.params_changed()
        label = "%dx%d all five fields full" % (E, N)
        assert tp.needed_widths([env.t[n].cpu().numpy() for n in tp.COLUMNS]) == tp.WIDTHS
        bad += _pack_matches(label, env)
        bad += _all_ones_fields(label, env, tops)
        bad += _rollout_matches(label, env, reset=False, counts=(2, 70))
        for name in tp.COLUMNS:
            env.t[name].copy_(orig[name])
        env.params_changed()
        bad += _pack_matches("%dx%d restored" % (E, N), env)
        for name in tp.COLUMNS:
            if not _same_bits(env.t[name], orig[name]):
                bad.append("%dx%d restored: %s differs" % (E, N, name))
    return bad


MODES = {"forms": (_mode_forms, {"MDR_ROLLOUT_STREAM_HOUSES": "0"}),
         "pack_off": (_mode_pack_off, {"MDR_ROLLOUT_STREAM_HOUSES": "0", "MDR_THERMAL_PACK": "0"}),
         "unset": (_mode_unset, {}),
         "extras": (_mode_extras, {"MDR_ROLLOUT_STREAM_HOUSES": "0"}),
         "edges": (_mode_edges, {"MDR_ROLLOUT_STREAM_HOUSES": "0"})}


def _run_child(mode, arg="-"):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(MODES[mode][1])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode, arg], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and "thermal pack ok: %s %s" % (mode, arg) in p.stdout, "%s %s (rc %s):\n%s" % (mode, arg, p.returncode, p.stdout[-3000:])


@pytest.mark.parametrize("controller", ("bangbang", "deadband", "external"))
def test_packed_rollout_leaves_what_single_steps_leave(controller):
    _run_child("forms", controller)


def test_fallback_constructor_switch_and_snapshot():
    _run_child("extras")


def test_pack_switched_off_in_the_environment():
    _run_child("pack_off")


def test_unset_threshold_takes_the_parents_plan_at_small_shapes():
    _run_child("unset")


def test_fields_exactly_full_and_ranges_one_pattern_too_wide():
    _run_child("edges")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    mode, arg = sys.argv[1], sys.argv[2]
    mismatches = MODES[mode][0](arg)
    if mismatches:
        print("\n".join(mismatches))
        sys.exit(1)
    print("thermal pack ok: %s %s" % (mode, arg))
