"""mdr_env_rollout's interior steps (MDR_ROLLOUT_INTERIOR = 0 | 1 | 2): steps 0 .. K - 2 of rollout(K) run the interior form of
k_step_fused / k_step_group, which leaves out the outputs the next launch overwrites (depth 1: reward, obs planes 5 / 6, actions, P and
the reduction behind them; depth 2: the five local planes too); the last step is a full one.  Whatever the depth, rollout(K) must leave
what K single steps leave, bit for bit: Ta, Tm, sso, flags, actions, reward, P and all seven obs planes.

The depth is read once per process, so every test starts one fresh child per depth (this file run as a script, never an exec) and
the three run side by side; a child builds each env once per case, fills the outputs with a sentinel, and compares rollout(K) on the
env with K x step_controller() / step(actions) on a deep copy of it."""
import copy
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = (0, 1, 2)
STEP_COUNTS = (1, 2, 3, 19)          # table_steps = 8: 19 steps cross two refills
TABLE_STEPS = 8
E = 3
# the smallest N that reaches each form and leaves a ragged last tile (profiles/plan_oracle_README.md); 1024: the benchmark's form
FUSED_SHAPES = {65: "k_step_fused<1,1,256>", 257: "k_step_fused<1,2,256>", 132: "k_step_fused<4,1,64>", 260: "k_step_fused<4,1,128>",
                516: "k_step_fused<4,1,256>", 1028: "k_step_fused<4,2,256>", 1024: "k_step_fused<4,1,256>"}
# the group form: N = 20 and 50 at 3 envs run one house per lane; 66 houses run two per lane and 68 four, both with idle lanes
GROUP_SHAPES = {(20, E): "k_step_group<32,1>", (50, E): "k_step_group<64,1>", (66, E): "k_step_group<64,2>", (68, E): "k_step_group<32,4>"}
SENTINEL_F, SENTINEL_B = -12345.0, 171
COMPARED = ("Ta", "Tm", "sso", "flags", "actions", "reward", "P", "obs")


def _cfg(N, mode="individual_L2", **patches):
    import mdr_amd
    cfg = mdr_amd.default_config()
    env = cfg["default_env_prop"]
    env["cluster_prop"]["nb_agents"] = N
    env["power_grid_prop"]["base_power_mode"] = "constant"
    env["power_grid_prop"]["signal_mode"] = "perlin"
    env["reward_prop"]["temp_penalty_mode"] = mode
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    for dotted, v in patches.items():
        node = cfg
        parts = dotted.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


def _prefill(env):
    """What an interior step must not be caught leaving behind: every output holds a sentinel before the call."""
    for k in ("reward", "obs", "P"):
        env.t[k].fill_(SENTINEL_F)
    env.t["actions"].fill_(SENTINEL_B)


def _check(label, cfg, controller="bangbang", external=False, planes=True, form=None, E=E, **kw):
    """rollout(K) against K single steps on a deep copy, for every K; returns the list of mismatches."""
    import torch
    import mdr_amd
    from tests import plan_util as pu
    N = cfg["default_env_prop"]["cluster_prop"]["nb_agents"]
    if form is not None:
        assert pu.step_kernel(N, E) == form, (label, pu.step_kernel(N, E), form)      # the case reaches the form it is there for
    make_exchange = kw.pop("make_exchange", None)      # an exchange object is per env and a deep copy does not carry it: the replica is built the same way

    def build():
        extra = {} if make_exchange is None else {"exchange": make_exchange()}
        e = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=7, table_steps=TABLE_STEPS, **kw, **extra)
        e.set_controller(controller)
        return e

    env = build()
    twin = None if make_exchange is None else build()
    bad = []
    for K in STEP_COUNTS:
        env.reset(episode=0)
        if twin is None:
            ref = copy.deepcopy(env)
        else:
            ref = twin
            ref.reset(episode=0)
        if not planes:
            env.set_obs_planes(False)
            ref.set_obs_planes(False)
        _prefill(env)
        _prefill(ref)
        act = None
        if external:
            act = (torch.rand((E, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(K)) < 0.6).to(torch.uint8)
        for _ in range(K):
            ref.step(act) if external else ref.step_controller()
        env.rollout(K, act)
        torch.cuda.synchronize()
        assert env.steps_taken == ref.steps_taken == K
        for k in COMPARED:
            a, b = env.t[k], ref.t[k]
            same = torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.numel() else a.numel() == b.numel()      # bits, so that NaN == NaN
            if not same:
                bad.append("%s K=%d %s: %d of %d elements differ" % (label, K, k, int((a != b).sum()), a.numel()))
        if planes and not external:      # a full last step overwrote every sentinel
            assert not bool((env.t["reward"] == SENTINEL_F).any()) and not bool((env.t["actions"] == SENTINEL_B).any()), label
        if not planes:
            env.set_obs_planes(True)
    return bad


def _group_forms():
    bad = []
    for N, form in FUSED_SHAPES.items():
        bad += _check("N=%d %s" % (N, form), _cfg(N), form=form)
    for (N, envs), form in GROUP_SHAPES.items():
        bad += _check("N=%d E=%d %s" % (N, envs, form), _cfg(N), form=form, E=envs)
    return bad


def _group_controllers():
    bad = []
    for N in (516, 20):
        for ctl in ("bangbang", "deadband", "always_on"):
            bad += _check("N=%d %s" % (N, ctl), _cfg(N), controller=ctl)
        bad += _check("N=%d external actions" % N, _cfg(N), external=True)
    return bad


def _group_penalties():
    bad = []
    for mode in ("individual_L2", "common_L2", "common_max", "mixture"):
        for N in (260, 20):
            bad += _check("N=%d %s" % (N, mode), _cfg(N, mode))
    return bad


def _group_noplanes():
    bad = []
    for N in (516, 20):
        bad += _check("N=%d planes off" % N, _cfg(N), planes=False)
        bad += _check("N=%d planes off, external actions" % N, _cfg(N), planes=False, external=True)
    return bad


def _group_full_steps():
    """Paths that must not take the interior form: something looks between the steps, or the step form has none."""
    from mdr_amd.sharding import MailboxExchange
    from tests import golden_util as gu
    bad = _check("sharded houses (a world of one)", _cfg(516), house_shard=(0, 516), exchange_always=True, make_exchange=MailboxExchange)
    bad += _check("graph mode", _cfg(516), graph_mode=True)
    bad += _check("graph mode, group form", _cfg(20), graph_mode=True)
    interp = {"default_env_prop.power_grid_prop.base_power_mode": "interpolation", "default_env_prop.time_step": 60}
    grid = gu.Golden("s12_interp_default_like").interp_grid()
    bad += _check("interpolated base power", _cfg(40, **interp), interp_grid=grid)      # an update every 5 steps
    bad += _check("interpolated base power, fused form", _cfg(516, **interp), interp_grid=grid)
    bad += _check("split step (k_step_partial + k_step_finish)", _cfg(1025), form="k_step_partial<1,256>+k_step_finish<1,256>")
    return bad


GROUPS = {"forms": _group_forms, "controllers": _group_controllers, "penalties": _group_penalties, "noplanes": _group_noplanes,
          "full_steps": _group_full_steps}


def _run_children(group):
    procs = []
    for d in DEPTHS:
        env = dict(os.environ, MDR_ROLLOUT_INTERIOR=str(d))
        procs.append((d, subprocess.Popen([sys.executable, os.path.abspath(__file__), group], cwd=ROOT, env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = []
    for d, p in procs:
        out, _ = p.communicate(timeout=300)
        if p.returncode != 0 or "interior ok: %s depth %d" % (group, d) not in out:
            failed.append("depth %d (rc %s):\n%s" % (d, p.returncode, out[-3000:]))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_rollout_leaves_what_single_steps_leave_at_every_depth(group):
    _run_children(group)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    group = sys.argv[1]
    depth = os.environ["MDR_ROLLOUT_INTERIOR"]
    mismatches = GROUPS[group]()
    if mismatches:
        print("\n".join(mismatches))
        sys.exit(1)
    print("interior ok: %s depth %s" % (group, depth))
