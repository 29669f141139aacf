"""The device-side minibatch indices as restated in tests/minibatch_ref.py (no GPU): the permutation is one, it moves with epoch,
seed and cursor, wrong variants give other integers, positions and values are independent by a chi-square test on pinned seeds; the
host-only correction table equals mdr_adam_step's two expressions; the new entry points refuse bad arguments before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

from mdr_amd import _native as nat
from tests import minibatch_ref as mr

SEED = 0x1234567890ABCDEF


@pytest.mark.parametrize("n", list(range(1, 601)) + [4095, 4096, 4097, 65537])
def test_permutation_is_a_bijection(n):
    p = mr.permutation(n, SEED, 3)
    assert p.dtype == np.int64 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n))


def test_half_width_follows_the_pinned_definition():
    assert [mr.half_width(n) for n in (1, 2, 3, 4, 5, 16, 17, 256, 257, 4097, 65537)] == [1, 1, 1, 1, 2, 2, 3, 4, 5, 7, 9]
    for n in (2, 3, 5, 300, 4097, 70001):
        assert 4 ** mr.half_width(n) < 4 * n      # the domain stays below 4 n: a few rounds of cycle walking on average


def test_permutation_differs_between_epochs_and_seeds():
    n = 300
    base = mr.permutation(n, SEED, 0)
    assert not np.array_equal(base, mr.permutation(n, SEED, 1))
    assert not np.array_equal(base, mr.permutation(n, SEED + 1, 0))
    assert not np.array_equal(base, mr.permutation(n, SEED ^ (1 << 40), 0))      # the key's high word
    assert not np.array_equal(base, mr.permutation(n, SEED, 1 << 32))            # the epoch's high word
    assert np.array_equal(base, mr.permutation(n, SEED, 0))


def test_cursor_adds_to_the_epoch():
    assert np.array_equal(mr.permutation(300, SEED, 5, cursor=4), mr.permutation(300, SEED, 9))
    # ... to its low word alone, mod 2^32, with no carry into the high word
    assert np.array_equal(mr.permutation(300, SEED, (7 << 32) | 0xFFFFFFFF, cursor=2), mr.permutation(300, SEED, (7 << 32) | 1))
    assert np.array_equal(mr.sample(64, 1000, SEED, 5, cursor=4), mr.sample(64, 1000, SEED, 9))


def test_wrong_variants_give_other_integers():
    """Three rounds, or another half width, is still a bijection - only a comparison of the integers catches it."""
    for n in (257, 4097):
        right = mr.permutation(n, SEED, 2)
        for wrong in (mr.permutation(n, SEED, 2, rounds=3), mr.permutation(n, SEED, 2, half_bits=mr.half_width(n) + 1)):
            assert np.array_equal(np.sort(wrong), np.arange(n))
            assert (wrong != right).mean() > 0.9


def test_position_and_value_are_independent():
    """n = 5120, 64 epochs, the 16 x 16 table of (position bucket, value bucket) counts: every cell expects 64 * 5120 / 256 = 1280,
    the row and column sums are exact by construction (a permutation), so Pearson's statistic has 15 * 15 = 225 degrees of freedom.
    Deterministic: the seeds are pinned."""
    n, epochs, K = 5120, 64, 16
    counts = np.zeros((K, K), dtype=np.int64)
    pos = np.arange(n) // (n // K)
    for epoch in range(epochs):
        val = mr.permutation(n, 20240607, epoch) // (n // K)
        np.add.at(counts, (pos, val), 1)
    expect = epochs * n / (K * K)
    stat = float(((counts - expect) ** 2 / expect).sum())
    limit = mr.chi_square_quantile(0.999, 225)
    print("Pearson statistic %.1f, 0.999 quantile of chi-square(225) %.1f" % (stat, limit))
    assert 295.0 < limit < 298.0      # 225 + 3.09 sqrt(450) = 290.5 by the normal approximation, the skew adds about 6
    assert stat < limit


def test_sample_stays_below_the_length_and_covers_it():
    for nb, length in ((1, 1), (256, 256), (256, 257), (1000, 524288), (4096, 3)):
        s = mr.sample(nb, length, SEED, 11)
        assert s.shape == (nb,) and s.min() >= 0 and s.max() < length
    s = mr.sample(4096, 3, SEED, 11)
    assert all(abs((s == k).mean() - 1 / 3) < 0.05 for k in range(3))
    assert not np.array_equal(mr.sample(256, 1000, SEED, 0), mr.sample(256, 1000, SEED, 1))
    assert not np.array_equal(mr.sample(256, 1000, SEED, 0), mr.sample(256, 1000, SEED + 1, 0))


@pytest.mark.parametrize("first", [1, 2, 1000, 10 ** 6])
def test_adam_corrections_are_the_two_host_expressions(first):
    lib = nat.load()
    lr, b1, b2, count = 3e-3, 0.9, 0.999, 5
    out = (C.c_float * (2 * count))()
    assert lib.mdr_adam_corrections(lr, b1, b2, first, count, out) == nat.MDR_OK
    for k in range(count):
        step = first + k
        assert out[2 * k] == np.float32(lr / (1.0 - math.pow(b1, float(step))))
        assert out[2 * k + 1] == np.float32(math.sqrt(1.0 - math.pow(b2, float(step))))


def test_adam_corrections_refuse():
    lib = nat.load()
    out = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    for args in ((1e-3, 0.9, 0.999, 1, 2, None), (1e-3, 0.9, 0.999, 0, 2, out), (1e-3, 0.9, 0.999, 1, -1, out), (float("nan"), 0.9, 0.999, 1, 2, out),
                 (1e-3, 1.0, 0.999, 1, 2, out), (1e-3, 0.9, -0.1, 1, 2, out)):
        assert lib.mdr_adam_corrections(*args) == nat.MDR_ERR_INVALID, args
    assert list(out) == [7.0] * 4
    assert lib.mdr_adam_corrections(1e-3, 0.9, 0.999, 1, 0, out) == nat.MDR_OK and list(out) == [7.0] * 4


def test_minibatch_calls_refuse_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
    assert lib.mdr_minibatch_permutation(-1, 0, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_permutation(16, 0, 0, None, None, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_permutation(1 << 62, 0, 0, None, p, None) == nat.MDR_ERR_UNSUPPORTED
    assert lib.mdr_minibatch_permutation(0, 0, 0, None, None, None) == nat.MDR_OK      # nothing to launch
    assert lib.mdr_minibatch_permutation_keyed(16, None, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_permutation_keyed(-1, p, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(-1, None, 10, 0, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(16, None, 10, 0, 0, None, None, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(16, None, 0, 0, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(16, None, -5, 0, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(16, None, 1 << 32, 0, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_minibatch_sample(0, None, 10, 0, 0, None, None, None) == nat.MDR_OK
    assert lib.mdr_minibatch_sample_keyed(16, None, 10, None, 0, None, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_set(None, 1, 0, 0, 0, 0, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_set(p, 0, 0, 0, 0, 0, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_set(p, 5, 0, 0, 0, 0, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_set(p, -1, 0, 0, 0, 0, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_add(None, 0, 1, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_update_cursor_add(p, -1, 1, None) == nat.MDR_ERR_INVALID


def test_adam_step_table_refuses_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    table = nat.MdrAdamSegments()
    table.struct_size = C.sizeof(nat.MdrAdamSegments)
    table.nb_segments = 0

    def call(seg=table, m=p, v=p, lr=1e-3, b1=0.9, corr=p, slot=0, base=None, clamp=math.inf):
        return lib.mdr_adam_step_table(C.byref(seg) if seg is not None else None, m, v, lr, b1, 0.999, 1e-8, corr, slot, base, 0.5, clamp, 0.0, None,
                                       None, 0, None)

    for kw in (dict(corr=None), dict(slot=-1), dict(seg=None), dict(m=None), dict(v=None), dict(b1=1.0), dict(lr=float("nan")), dict(clamp=-1.0)):
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    assert call() == nat.MDR_OK      # no segments, no norm asked for: nothing to launch
    assert len(lib.mdr_adam_step_table.argtypes) == len(lib.mdr_adam_step.argtypes) + 2
