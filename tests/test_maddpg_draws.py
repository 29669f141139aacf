"""The device-side draws of one MADDPG update as restated in tests/maddpg_draws_ref.py (no GPU): every agent's minibatch is distinct
positions below the buffer's length, the draws move with seed, step and cursor, wrong variants give other integers, the gumbel noise
is finite with Gumbel(0, 1)'s mean and variance; the entry points refuse bad arguments before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

from mdr_amd import _native as nat
from tests import maddpg_draws_ref as dr

SEED = 0x1234567890ABCDEF
SHAPES = [(1, 1, 1), (3, 5, 5), (3, 16, 17), (20, 64, 64), (20, 64, 65), (4, 16, 257), (2, 64, 524288)]      # (N, B, len)


@pytest.mark.parametrize("N,B,length", SHAPES)
def test_every_row_is_distinct_positions_below_the_length(N, B, length):
    idx = dr.index(N, B, length, SEED, 3)
    assert idx.dtype == np.int64 and idx.shape == (N, B)
    assert idx.min() >= 0 and idx.max() < length
    for a in range(N):
        assert np.unique(idx[a]).size == B
    if B == length:      # the whole buffer: a permutation of it
        assert all(np.array_equal(np.sort(idx[a]), np.arange(length)) for a in range(N))


def test_rows_of_different_agents_differ():
    for N, B, length in ((3, 16, 17), (20, 64, 65), (4, 16, 257)):
        idx = dr.index(N, B, length, SEED, 3)
        for a in range(N):
            for b in range(a + 1, N):
                assert not np.array_equal(idx[a], idx[b]), (a, b)


def _both(seed, step, cursor=0):
    t, a = dr.noise(3, 16, seed, step, cursor)
    return dr.index(3, 16, 300, seed, step, cursor), t, a


def test_draws_move_with_seed_step_and_cursor():
    base = _both(SEED, 5)
    for other in (_both(SEED + 1, 5), _both(SEED ^ (1 << 40), 5), _both(SEED, 6), _both(SEED, 5 | (1 << 32)), _both(SEED, 5, cursor=1)):
        for x, y in zip(base, other):
            assert not np.array_equal(x, y)
    for x, y in zip(base, _both(SEED, 5)):
        assert np.array_equal(x, y)


def test_cursor_adds_to_the_low_word_without_carry():
    for x, y in zip(_both(SEED, 5, cursor=4), _both(SEED, 9)):
        assert np.array_equal(x, y)
    for x, y in zip(_both(SEED, (7 << 32) | 0xFFFFFFFF, cursor=2), _both(SEED, (7 << 32) | 1)):
        assert np.array_equal(x, y)
    for x, y in zip(_both(SEED, (7 << 32) | 0xFFFFFFFF, cursor=2), _both(SEED, (8 << 32) | 1)):
        assert not np.array_equal(x, y)


def test_wrong_variants_give_other_integers():
    """Three rounds, or another half width, still gives distinct positions - only a comparison of the integers catches it."""
    for length in (257, 4097):
        right = dr.index(2, length, length, SEED, 2)
        for wrong in (dr.index(2, length, length, SEED, 2, rounds=3), dr.index(2, length, length, SEED, 2, half_bits=dr.half_width(length) + 1)):
            assert all(np.array_equal(np.sort(wrong[a]), np.arange(length)) for a in range(2))
            assert (wrong != right).mean() > 0.9


def test_noise_is_gumbel():
    """N = 4, B = 2500: 4 x 2500 x 5 x 2 = 10^5 values, 80000 of the targets' and 20000 of the actors'.  The
    mean's standard deviation is 1.283 / sqrt(10^5) = 0.004, so 0.016 is 4 sigma; the sample variance's is sqrt((mu4 - sigma^4) / n) with
    Gumbel's mu4 = 5.4 sigma^4 (excess kurtosis 12 / 5): sqrt(4.4 x 2.7058 / 10^5) = 0.0109, so 0.05 is 4.6 sigma."""
    N, B = 4, 2500
    words = dr.noise_words(N, B, 20240607, 11)
    g64 = dr.gumbel(words)
    t, a = dr.noise(N, B, 20240607, 11)
    assert t.dtype == np.float32 and t.shape == (N, B, N, 2) and a.shape == (N, B, 2)
    g = np.concatenate([t.ravel(), a.ravel()]).astype(np.float64)
    assert g.size == 100000
    assert np.isfinite(g).all() and g.min() >= -3.2 and g.max() <= 23.0
    mean, var = g.mean(), g.var(ddof=1)
    print("mean %.5f (0.5772 +- 0.016), variance %.5f (%.5f +- 0.05)" % (mean, var, math.pi ** 2 / 6))
    assert abs(mean - 0.5772) < 0.016
    assert abs(var - math.pi ** 2 / 6) < 0.05
    assert np.array_equal(np.concatenate([t, a[:, :, None]], 2), g64.astype(np.float32))
    # noise_t and noise_a of one call share no word: the counter q is distinct for every pair
    assert np.unique(words.reshape(-1, 2), axis=0).shape[0] == N * B * (N + 1)
    assert not np.isin(words[:, :, N].ravel(), words[:, :, :N].ravel()).any()


def test_the_extreme_words_stay_finite_in_double():
    g = dr.gumbel(np.array([0, 1, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)).astype(np.float32)
    assert np.isfinite(g).all() and g.min() > -3.2 and g.max() < 23.0
    # ... which fp32 would not: u rounds to 1.0 for the top words
    assert np.float32((np.float32(0xFFFFFFFF) + np.float32(0.5)) / np.float32(4294967296.0)) == np.float32(1.0)


def _draws(lib, N=3, B=4, len_dev=None, length=10, idx=1, nt=1, na=1):
    p = C.c_void_p(0x1000)      # never dereferenced: every refused call returns before a launch
    return lib.mdr_maddpg_draws(N, B, len_dev, length, 0, 0, None, p if idx else None, p if nt else None, p if na else None, None)


def test_draws_refuse_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    assert _draws(lib, idx=0) == nat.MDR_ERR_INVALID
    assert _draws(lib, nt=0) == nat.MDR_ERR_INVALID
    assert _draws(lib, na=0) == nat.MDR_ERR_INVALID
    assert _draws(lib, N=0) == nat.MDR_ERR_INVALID
    assert _draws(lib, N=-1) == nat.MDR_ERR_INVALID
    assert _draws(lib, B=-1) == nat.MDR_ERR_INVALID
    assert _draws(lib, length=0) == nat.MDR_ERR_INVALID
    assert _draws(lib, length=-3) == nat.MDR_ERR_INVALID
    assert _draws(lib, B=11, length=10) == nat.MDR_ERR_INVALID      # no 11 distinct positions among 10
    assert nat.MDR_MADDPG_DRAWS_MAX_AGENTS == dr.MAX_AGENTS == 1280 // 3
    assert _draws(lib, N=dr.MAX_AGENTS + 1) == nat.MDR_ERR_UNSUPPORTED
    assert _draws(lib, length=1 << 62) == nat.MDR_ERR_UNSUPPORTED
    assert _draws(lib, B=0) == nat.MDR_OK      # nothing to launch
    assert _draws(lib, B=0, idx=0, nt=0, na=0) == nat.MDR_OK
    assert lib.mdr_maddpg_draws_keyed(3, 4, None, 10, None, 0, None, p, p, p, None) == nat.MDR_ERR_INVALID      # no key
    assert lib.mdr_maddpg_draws_keyed(3, 11, None, 10, p, 0, None, p, p, p, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_maddpg_draws_keyed(3, 0, None, 10, p, 0, None, p, p, p, None) == nat.MDR_OK


def test_tags_are_the_headers():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdr_policy.h")) as f:
        text = f.read()
    tags = dict(re.findall(r"#define (MDR_TAG_MADDPG_[A-Z]+) (0x[0-9A-Fa-f]+)u", text))
    assert int(tags["MDR_TAG_MADDPG_INDEX"], 16) == dr.TAG_INDEX == int.from_bytes(b"MDI1", "big")
    assert int(tags["MDR_TAG_MADDPG_NOISE"], 16) == dr.TAG_NOISE == int.from_bytes(b"MDN1", "big")


def test_constructor_refusals_that_need_no_gpu():
    """The sampler's name is checked before anything touches the networks."""
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
    actor, critic = DDPGNetworkMLP(4, 2, 8), DDPGNetworkMLP(2 * 6, 1, 8)
    with pytest.raises(ValueError, match="sampler"):
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=8, sampler="numpy")
    with pytest.raises(ValueError, match="graph=True"):      # backend='torch' is refused before a graph could be built
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=8, backend="torch", graph=True)
    with pytest.raises(ValueError, match="graph=True"):
        MADDPGLearner(actor, critic, 2, 1e-3, 1e-3, buffer_capacity=8, backend="auto", sampler="torch", graph=True)
