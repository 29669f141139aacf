"""The integer algebra behind the lean per-step update of the resident rollout kernels (house_advance_lean_m / house_lock_m in
csrc/mdr_device.h), restated in NumPy and checked exhaustively - no GPU.

The HVAC's state machine (env 475-492; house_advance_m) per step, with `on`, `cmd` booleans and sso the seconds since it went off:

    general                                       lean (needs on => sso == 0 on entry)
    sso1 = sso if on else sso + dt                t    = sso + dt
    can  = on or sso1 >= lockout                  can  = on or t >= lockout
    on2  = can and cmd                            on2  = can and cmd
    sso2 = 0 if on2 else sso1                     sso2 = 0 if (on or on2) else t
    lock = not can or (not on2 and sso2 + dt < lockout)          - the same expression, evaluated where it is read

(a) one general step establishes the invariant, (b) under it the lean step is the general step, (c) a launch of n steps - one
general, n - 1 lean, the lock formed once behind the last from that step's `can` and the sso it left - ends where n general steps
with a per-step lock end.  The grid: on, cmd in {0, 1}, dt in {1, 4}, lockout in {0, dt, 3 dt, 3 dt + 1}, sso in [0, lockout + 2 dt]."""
import itertools

import numpy as np
import pytest

DTS = (1, 4)
STEP_COUNTS = (1, 2, 5)


def general_step(sso, on, cmd, lockout, dt):
    sso1 = np.where(on, sso, sso + dt)
    can = on | (sso1 >= lockout)
    on2 = can & cmd
    sso2 = np.where(on2, 0, sso1)
    lock = ~can | (~on2 & (sso2 + dt < lockout))
    return sso2, on2, can, lock


def lean_step(sso, on, cmd, lockout, dt):
    t = sso + dt
    can = on | (t >= lockout)
    on2 = can & cmd
    sso2 = np.where(on | on2, 0, t)
    return sso2, on2, can


def lock_behind(can, on2, sso2, lockout, dt):
    return ~can | (~on2 & (sso2 + dt < lockout))


def grid(dt):
    """Every (sso, on, lockout) of the issue's grid for one dt, as three flat arrays."""
    rows = [(s, on, L) for L in (0, dt, 3 * dt, 3 * dt + 1) for on in (False, True) for s in range(L + 2 * dt + 1)]
    sso, on, lockout = (np.array(c) for c in zip(*rows))
    return sso.astype(np.int32), on.astype(bool), lockout.astype(np.int32)


@pytest.mark.parametrize("dt", DTS)
def test_one_general_step_leaves_on_only_with_sso_zero(dt):
    sso, on, lockout = grid(dt)
    assert (on & (sso != 0)).any()      # the grid holds entry states that break the invariant
    for cmd in (False, True):
        sso2, on2, _, _ = general_step(sso, on, np.full(on.shape, cmd), lockout, dt)
        assert not (on2 & (sso2 != 0)).any()


@pytest.mark.parametrize("dt", DTS)
def test_under_the_invariant_the_lean_step_is_the_general_step(dt):
    sso, on, lockout = grid(dt)
    ok = ~on | (sso == 0)
    sso, on, lockout = sso[ok], on[ok], lockout[ok]
    assert on.any() and (~on).any() and (sso > lockout).any()
    for cmd in (False, True):
        c = np.full(on.shape, cmd)
        g_sso, g_on, g_can, g_lock = general_step(sso, on, c, lockout, dt)
        l_sso, l_on, l_can = lean_step(sso, on, c, lockout, dt)
        assert np.array_equal(g_sso, l_sso) and np.array_equal(g_on, l_on) and np.array_equal(g_can, l_can)
        assert np.array_equal(g_lock, lock_behind(l_can, l_on, l_sso, lockout, dt))


def test_the_lean_step_is_wrong_without_the_invariant():
    """The restatement can tell the two forms apart: from `on` with sso != 0 and no command the lean form loses the count."""
    sso, on, cmd, lockout = np.array([3]), np.array([True]), np.array([False]), np.array([0])
    assert general_step(sso, on, cmd, lockout, 1)[0][0] == 3 and lean_step(sso, on, cmd, lockout, 1)[0][0] == 0


@pytest.mark.parametrize("n", STEP_COUNTS)
@pytest.mark.parametrize("dt", DTS)
def test_the_lock_formed_behind_the_last_of_n_steps_is_that_steps_lock(dt, n):
    sso0, on0, lockout = grid(dt)
    for cmds in itertools.product((False, True), repeat=n):      # every command sequence, the same for all states of the grid
        sso, on = sso0.copy(), on0.copy()
        l_sso, l_on = sso0.copy(), on0.copy()
        for s, cmd in enumerate(cmds):
            c = np.full(on.shape, cmd)
            sso, on, _, lock = general_step(sso, on, c, lockout, dt)
            if s == 0:
                l_sso, l_on, l_can, _ = general_step(l_sso, l_on, c, lockout, dt)
            else:
                l_sso, l_on, l_can = lean_step(l_sso, l_on, c, lockout, dt)
        assert np.array_equal(sso, l_sso) and np.array_equal(on, l_on), (dt, cmds)
        assert np.array_equal(lock, lock_behind(l_can, l_on, l_sso, lockout, dt)), (dt, cmds)
