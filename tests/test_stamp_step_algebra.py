"""The integer algebra behind the time-stamp form of the resident rollout loop (house_advance_stamp_m in csrc/mdr_device.h, taken by
k_rollout_resident* where one lockout L holds for every house), restated in NumPy and checked exhaustively - no GPU.

The HVAC's state machine per step (env 475-492; house_advance), with sso the seconds since the HVAC went off:

    general                                       stamp form, step s >= 1 of a launch: from Ts = s dt to Tn = Ts + dt
    sso1 = sso if on else sso + dt
    can  = on or sso1 >= L                        can = on or z <= Ts - L
    on2  = can and cmd                            on2 = can and cmd
    sso2 = 0 if on2 else sso1                     z2  = Tn if on2 else z
    lock = not can or (not on2 and sso2 + dt < L)

z is the end of the last step that left the HVAC on: at the start of a step an `on` house has z = Ts, an `off` one sso = Ts - dt - z.
A launch of n steps runs step 0 in the general form, sets z = dt if on else -sso behind it (house_stamp at T = dt), runs steps
1 .. n - 1 in the stamp form, and behind the last forms sso = max(0, n dt - dt - z) (house_stamp_sso) and from it the lock
(house_lock_m).  For every prefix of every command sequence that must be what n general steps leave: `on`, `can`, `sso` and `lock`.

The grid: dt in {1, 4}; L in {0, dt, 2 dt, 5 dt, 10 dt}; entry sso in {0, 1, L - 2 dt, L - dt, L, L + dt, 10^6} (clamped at 0); entry
on / off - an `on` house with sso != 0 included, which is why step 0 keeps the general form; every command sequence of length 8 with
all its prefixes, and seeded random sequences of length 40."""
import itertools

import numpy as np
import pytest

DTS = (1, 4)
LENGTH = 8
LONG, LONG_RUNS = 40, 6


def general_step(sso, on, cmd, lockout, dt):
    sso1 = np.where(on, sso, sso + dt)
    can = on | (sso1 >= lockout)
    on2 = can & cmd
    sso2 = np.where(on2, 0, sso1)
    lock = ~can | (~on2 & (sso2 + dt < lockout))
    return sso2, on2, can, lock


def stamp_step(z, on, cmd, lockout, Tn, dt):
    can = on | (z <= Tn - dt - lockout)
    on2 = can & cmd
    return np.where(on2, Tn, z), on2, can


def lock_behind(can, on2, sso2, lockout, dt):
    return ~can | (~on2 & (sso2 + dt < lockout))


def grid(dt):
    """Every (sso, on, L) of the grid for one dt, as three flat int64 / bool arrays."""
    rows = []
    for L in (0, dt, 2 * dt, 5 * dt, 10 * dt):
        for sso in (0, 1, L - 2 * dt, L - dt, L, L + dt, 10 ** 6):
            for on in (False, True):
                rows.append((max(sso, 0), on, L))
    sso, on, lockout = (np.array(c) for c in zip(*rows))
    return sso.astype(np.int64), on.astype(bool), lockout.astype(np.int64)


def check_every_prefix(dt, cmds, stamp=stamp_step):
    """Runs `cmds` over the whole grid in both forms; returns the (prefix length, field) pairs that differ."""
    sso, on, lockout = grid(dt)
    g_sso, g_on = sso.copy(), on.copy()
    differ = []
    for s, cmd in enumerate(cmds):
        c = np.full(on.shape, bool(cmd))
        g_sso, g_on, g_can, g_lock = general_step(g_sso, g_on, c, lockout, dt)
        if s == 0:
            l_sso, l_on, l_can, _ = general_step(sso, on, c, lockout, dt)
            z = np.where(l_on, dt, -l_sso)
        else:
            z, l_on, l_can = stamp(z, l_on, c, lockout, (s + 1) * dt, dt)
        n = s + 1      # a launch that ends here
        end_sso = np.maximum(0, n * dt - dt - z)
        fields = {"on": (g_on, l_on), "can": (g_can, l_can), "sso": (g_sso, end_sso), "lock": (g_lock, lock_behind(l_can, l_on, end_sso, lockout, dt))}
        differ += [(n, k) for k, (want, got) in fields.items() if not np.array_equal(want, got)]
    return differ


def test_the_grid_holds_the_states_it_is_there_for():
    for dt in DTS:
        sso, on, lockout = grid(dt)
        assert (on & (sso != 0)).any() and (~on & (sso == 0)).any()      # an `on` house with a count: step 0 must be general
        assert (sso == 10 ** 6).any() and (lockout == 0).any() and (sso > lockout).any() and ((sso < lockout) & ~on).any()


@pytest.mark.parametrize("dt", DTS)
def test_every_prefix_of_every_command_sequence_of_length_8(dt):
    for cmds in itertools.product((False, True), repeat=LENGTH):
        assert check_every_prefix(dt, cmds) == [], (dt, cmds)


@pytest.mark.parametrize("dt", DTS)
def test_random_command_sequences_of_length_40(dt):
    rng = np.random.default_rng(20 + dt)
    for run in range(LONG_RUNS):
        cmds = rng.random(LONG) < (0.15, 0.5, 0.85)[run % 3]      # mostly off, even, mostly on: long waits, many switches
        assert check_every_prefix(dt, cmds) == [], (dt, run)


def test_the_restatement_tells_wrong_forms_apart():
    """Three slips the stamp form invites, each visible on this grid."""
    def reset_by_on_or_on2(z, on, cmd, lockout, Tn, dt):      # the counter form's mask: a house switched off would count from the step's end
        can = on | (z <= Tn - dt - lockout)
        on2 = can & cmd
        return np.where(on | on2, Tn, z), on2, can

    def end_time_in_the_test(z, on, cmd, lockout, Tn, dt):      # z <= Tn - L: ready one step early
        can = on | (z <= Tn - lockout)
        on2 = can & cmd
        return np.where(on2, Tn, z), on2, can

    def strict_compare(z, on, cmd, lockout, Tn, dt):      # sso + dt > L
        can = on | (z < Tn - dt - lockout)
        on2 = can & cmd
        return np.where(on2, Tn, z), on2, can

    cmds = (True, True, False, False, False, True, True, True)
    assert check_every_prefix(4, cmds) == []
    for wrong in (reset_by_on_or_on2, end_time_in_the_test, strict_compare):
        assert check_every_prefix(4, cmds, stamp=wrong) != [], wrong.__name__
