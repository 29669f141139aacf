"""The thermal pack without a GPU: the entry points are exported and host-checked, and the format (tests/thermal_pack_ref.py) is
lossless on the oracle's own sample of the benchmark's configuration, needs the widths the field layout was chosen for at the
corners of house_big_noise's box, reports "not packed" for what it cannot hold, and is exact at the field boundary: a range of
2^w - 1 patterns fills field w with ones and touches no neighbour, a range of 2^w is refused."""
import itertools

import numpy as np
import pytest

import mdr_amd
from mdr_amd import _native as nat
from tests import thermal_pack_ref as tp

C3_NEEDS = (25, 25, 25, 26, 24)      # bits of max - min per column on the C3 sample and at the corners of the noise box


def _c3():
    import bench
    from oracle import mdr_oracle as mo
    ora = mo.OracleEnv(bench.c3_config(mdr_amd), nb_envs=16).reset(seed=2024, episode=0)
    return ora, tp.thermal_columns(ora.Ua, ora.Cm, ora.Ca, ora.Hm, ora.spec.dt)


@pytest.fixture(scope="module")
def c3():
    return _c3()


def test_entry_points_are_exported_and_host_checked():
    assert "mdr_env_bind_thermal_pack" in nat.EXPORTS and "mdr_env_rollout_plan" in nat.EXPORTS
    lib = mdr_amd.load_native()
    assert lib.mdr_env_bind_thermal_pack(None, None, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_env_rollout_plan(None, None, None) == nat.MDR_ERR_INVALID
    assert sum(nat.MDR_THERMAL_BITS) == 128 and len(nat.MDR_THERMAL_BITS) == 5
    assert all(w >= need for w, need in zip(nat.MDR_THERMAL_BITS, C3_NEEDS))
    assert nat.MDR_THERMAL_DESC_BASE + 5 <= nat.MDR_THERMAL_DESC_WORDS


def test_round_trip_is_bit_exact_on_the_c3_sample(c3):
    ora, cols = c3
    assert ora.E == 16 and ora.N == 1024
    packed, bases, planes = tp.pack(cols)
    assert packed and planes.shape == (4, 16 * 1024) and planes.dtype == np.uint32
    back = tp.unpack(bases, planes)
    for name, c, b in zip(tp.COLUMNS, cols, back):
        assert np.array_equal(tp.bits(c), tp.bits(b)), name
    assert all(n <= need for n, need in zip(tp.needed_widths(cols), C3_NEEDS)), tp.needed_widths(cols)


@pytest.mark.parametrize("dt", (1, 4, 60))
def test_corner_houses_need_the_c3_widths(c3, dt):
    """The 16 corners of house_big_noise's [0.5, 1.5]^4 box around the nominal house: the extremes of every column."""
    s = c3[0].spec
    corners = np.array(list(itertools.product((0.5, 1.5), repeat=4)))
    cols = tp.thermal_columns(s.Ua * corners[:, 0], s.Cm * corners[:, 1], s.Ca * corners[:, 2], s.Hm * corners[:, 3], dt)
    assert tp.needed_widths(cols) == C3_NEEDS
    packed, bases, planes = tp.pack(cols)
    assert packed
    for c, b in zip(cols, tp.unpack(bases, planes)):
        assert np.array_equal(tp.bits(c), tp.bits(b))


def test_not_packed_is_reported(c3):
    _, cols = c3
    flat = [c.ravel().copy() for c in cols]
    assert tp.describe(flat)[0]
    mixed = [c.copy() for c in flat]
    mixed[0][7] = -mixed[0][7]                                    # a column with both signs
    assert not tp.describe(mixed)[0] and tp.pack(mixed)[2] is None
    wide = [c.copy() for c in flat]
    wide[4][3] = np.float32(1.0 / (float(1.0 / wide[4][3]) * 1e-3))      # one house with Ua x 1e-3: inv_Ua leaves its field
    assert not tp.describe(wide)[0]
    nan = [c.copy() for c in flat]
    nan[2][0] = np.float32("nan")
    assert not tp.describe(nan)[0]
    neg_nan = [c.copy() for c in flat]                            # s0 is negative: a NaN with the sign set agrees in sign and is still refused
    neg_nan[1][0] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    assert not tp.describe(neg_nan)[0]


def test_a_column_holding_a_zero_still_packs_if_it_fits():
    n = 64
    tiny = (np.arange(n, dtype=np.uint32) * np.uint32(1000)).view(np.float32)      # +0.0 and subnormals: patterns 0 .. 63000
    cols = [tiny, tiny.copy(), np.zeros(n, dtype=np.float32), tiny.copy(), tiny.copy()]
    packed, bases, planes = tp.pack(cols)
    assert packed and int(bases[2]) == 0
    for c, b in zip(cols, tp.unpack(bases, planes)):
        assert np.array_equal(tp.bits(c), tp.bits(b))
    cols[2] = np.array([0.0] * (n - 1) + [1.0], dtype=np.float32)            # 0.0 next to 1.0: 0x3F800000 does not fit 25 bits
    assert not tp.describe(cols)[0]
    cols[2] = np.array([0.0] * (n - 1) + [-0.0], dtype=np.float32)           # -0.0 is another sign
    assert not tp.describe(cols)[0]


def _widened(flat, c, span):
    """The columns with one house of column c moved `span` patterns below the column's largest pattern (same sign, smaller
    magnitude): (columns, the house holding the largest pattern, the house written)."""
    cols = [x.copy() for x in flat]
    b = tp.bits(cols[c])
    top = int(b.argmax())
    hi = int(b[top])
    assert (hi & 0x7FFFFFFF) - span >= 0x00800000 and hi - span < int(b.min())      # still a normal number of that sign, and the new smallest
    house = (top + 1) % b.size
    cols[c].view(np.uint32)[house] = np.uint32(hi - span)
    return cols, top, house


@pytest.mark.parametrize("c", range(5))
def test_a_field_that_is_exactly_full_round_trips(c3, c):
    """max - min == 2^w - 1 in column c: still packed, the house with the largest pattern carries an all-ones field, the one with
    the smallest a zero, every column comes back bit for bit and the other four columns' fields are what they were."""
    flat = [x.ravel().copy() for x in c3[1]]
    w = tp.WIDTHS[c]
    before = tp.fields(tp.pack(flat)[2])
    cols, top, house = _widened(flat, c, (1 << w) - 1)
    assert tp.needed_widths(cols)[c] == w
    packed, bases, planes = tp.pack(cols)
    assert packed
    after = tp.fields(planes)
    assert int(after[c][top]) == (1 << w) - 1 and int(after[c][house]) == 0
    for j in range(5):
        if j != c:
            assert np.array_equal(after[j], before[j]), (tp.COLUMNS[c], tp.COLUMNS[j])      # an all-ones field leaks into no neighbour
    for name, col, back in zip(tp.COLUMNS, cols, tp.unpack(bases, planes)):
        assert np.array_equal(tp.bits(col), tp.bits(back)), name


@pytest.mark.parametrize("c", range(5))
def test_a_range_one_pattern_too_wide_is_not_packed(c3, c):
    flat = [x.ravel().copy() for x in c3[1]]
    cols, _, _ = _widened(flat, c, 1 << tp.WIDTHS[c])
    assert tp.needed_widths(cols)[c] == tp.WIDTHS[c] + 1
    assert not tp.describe(cols)[0] and tp.pack(cols)[2] is None


def test_all_five_fields_exactly_full_at_once(c3):
    flat = [x.ravel().copy() for x in c3[1]]
    cols, tops = flat, []
    for c in range(5):
        cols, top, house = _widened(cols, c, (1 << tp.WIDTHS[c]) - 1)
        tops.append(top)
    assert tp.needed_widths(cols) == tp.WIDTHS
    packed, bases, planes = tp.pack(cols)
    assert packed
    after = tp.fields(planes)
    assert [int(after[c][tops[c]]) for c in range(5)] == [(1 << w) - 1 for w in tp.WIDTHS]
    for name, col, back in zip(tp.COLUMNS, cols, tp.unpack(bases, planes)):
        assert np.array_equal(tp.bits(col), tp.bits(back)), name
