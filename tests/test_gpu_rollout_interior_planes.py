"""How many local obs planes mdr_env_rollout's interior steps still store (MDR_ROLLOUT_INTERIOR_PLANES = 0 .. 5, read once per
process): steps 0 .. K - 2 of rollout(K) run the interior form of k_step_fused / k_step_group that stores planes 0 .. count - 1 and
none of the outputs behind the env-wide reduction; the last step is a full one.  Whatever the count, rollout(K) must leave what K
single steps leave, bit for bit: Ta, Tm, sso, flags, actions, reward, P and all seven obs planes, every output prefilled with a
sentinel (tests/test_gpu_rollout_interior.py's comparison, whose helpers this file uses).

One fresh child per count (this file run as a script, never an exec), one after another, each under its own timeout; the first
child that does not end normally ends the test - nothing more is started on the device behind it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 2, 3, 4, 5)
E = 3
# the fused forms with a ragged last tile, and the group form at four houses per lane and at one
FUSED_SHAPES = {65: "k_step_fused<1,1,256>", 132: "k_step_fused<4,1,64>", 516: "k_step_fused<4,1,256>", 1028: "k_step_fused<4,2,256>"}
GROUP_SHAPES = {(20, E): "k_step_group<32,1>", (68, E): "k_step_group<32,4>"}
LOCKOUT_NOISE = {"default_hvac_prop.lockout_noise": 15}      # a `lockout` column that is streamed, not taken from element [0]
CHILD_TIMEOUT = 300


def _cases():
    import mdr_amd
    from tests.test_gpu_rollout_interior import TABLE_STEPS, _cfg, _check
    bad = []
    for N, form in FUSED_SHAPES.items():
        bad += _check("N=%d %s" % (N, form), _cfg(N), form=form)
    for (N, envs), form in GROUP_SHAPES.items():
        bad += _check("N=%d E=%d %s" % (N, envs, form), _cfg(N), form=form, E=envs)
    bad += _check("N=516 external actions", _cfg(516), external=True)
    bad += _check("N=516 planes off", _cfg(516), planes=False)
    for N in (516, 68):      # plane 4 divides by `lockout`, and the state advance reads it at every count
        cfg = _cfg(N, **LOCKOUT_NOISE)
        probe = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=7, table_steps=TABLE_STEPS)
        probe.reset(episode=0)
        assert probe.t["lockout"].unique().numel() > 1, "the lockout column of this case must not be uniform"
        bad += _check("N=%d non-uniform lockout" % N, cfg)
    return bad


def test_rollout_leaves_what_single_steps_leave_at_every_plane_count():
    for count in COUNTS:
        env = dict(os.environ, MDR_ROLLOUT_INTERIOR_PLANES=str(count))
        env.pop("MDR_ROLLOUT_INTERIOR", None)      # depth 1: the count decides
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
        ok = p.returncode == 0 and "interior planes ok: count %d" % count in p.stdout
        assert ok, "count %d (rc %s), later counts not run:\n%s" % (count, p.returncode, p.stdout[-3000:])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    mismatches = _cases()
    if mismatches:
        print("\n".join(mismatches))
        sys.exit(1)
    print("interior planes ok: count %s" % os.environ["MDR_ROLLOUT_INTERIOR_PLANES"])
