"""mdr_maddpg_draws on the GPU against tests/maddpg_draws_ref.py: the positions exactly - with a host or a device length, a host seed or
a device key, a cursor -, the gumbel noise to 1 float ulp with at least 99 % bit-equal (the double ``log`` is good to an ulp of double,
so the float can differ only on a rounding boundary), a device length below 1 read as 1, nothing stored past the outputs."""
import numpy as np
import pytest
import torch

from mdr_amd import graph_update as gu
from tests import maddpg_draws_ref as dr
from tests.test_maddpg_draws import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, STEP = 0x1234567890ABCDEF, (5 << 32) | 77


def _key(seed):
    return torch.tensor([gu._i32(seed), gu._i32(seed >> 32)], dtype=torch.int32, device=DEV)


def _check_noise(got_t, got_a, N, B, seed, step, cursor=0):
    want_t, want_a = dr.noise(N, B, seed, step, cursor)
    for got, want in ((got_t.cpu().numpy(), want_t), (got_a.cpu().numpy(), want_a)):
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.isfinite(got).all()
        ulp = np.spacing(np.abs(want))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        assert (got.view(np.uint32) == want.view(np.uint32)).mean() >= 0.99


@pytest.mark.parametrize("N,B,length", SHAPES + [(3, 5, 16), (3, 65, 256), (2, 65, 65)])
def test_draws_equal_the_restatement(N, B, length):
    """B = 5 and B = 65: a partial wave and a partial workgroup; len 16 / 17, 64 / 65, 256 / 257: either side of an h boundary."""
    want = dr.index(N, B, length, SEED, STEP)
    len_dev = torch.tensor([length], dtype=torch.int64, device=DEV)
    for length_arg in (length, len_dev):
        for key in (None, _key(SEED)):
            index, noise_t, noise_a = gu.maddpg_draws(N, B, length_arg, SEED if key is None else 0, STEP, DEV, key=key)
            assert index.dtype == torch.int64 and index.shape == (N, B)
            assert np.array_equal(index.cpu().numpy(), want)
            _check_noise(noise_t, noise_a, N, B, SEED, STEP)


def test_cursor_is_added_to_the_step():
    N, B, length = 3, 16, 300
    cursor = torch.tensor([3], dtype=torch.int32, device=DEV)
    with_cursor = gu.maddpg_draws(N, B, length, SEED, STEP, DEV, cursor=cursor)
    plain = gu.maddpg_draws(N, B, length, SEED, STEP + 3, DEV)
    for x, y in zip(with_cursor, plain):
        assert torch.equal(x, y)
    assert np.array_equal(plain[0].cpu().numpy(), dr.index(N, B, length, SEED, STEP + 3))
    assert np.array_equal(with_cursor[0].cpu().numpy(), dr.index(N, B, length, SEED, STEP, cursor=3))
    assert not torch.equal(plain[0], gu.maddpg_draws(N, B, length, SEED, STEP, DEV)[0])


@pytest.mark.parametrize("bad", [0, -7])
def test_a_device_length_below_one_is_one_and_nothing_is_stored_past_the_outputs(bad):
    N, B, pad = 3, 1, 64
    sizes = (N * B, N * B * N * 2, N * B * 2)
    raw = [torch.full((n + pad,), -12345, dtype=torch.int64, device=DEV) if k == 0 else torch.full((n + pad,), -12345.0, dtype=torch.float32, device=DEV)
           for k, n in enumerate(sizes)]
    out = (raw[0][:sizes[0]].view(N, B), raw[1][:sizes[1]].view(N, B, N, 2), raw[2][:sizes[2]].view(N, B, 2))
    gu.maddpg_draws(N, B, torch.tensor([bad], dtype=torch.int64, device=DEV), SEED, STEP, DEV, out=out)
    assert bool((out[0] == 0).all())      # len 1: every position is 0
    _check_noise(out[1], out[2], N, B, SEED, STEP)
    for buf, n in zip(raw, sizes):
        assert bool((buf[n:] == -12345).all())


def test_canaries_at_a_partial_workgroup():
    """N = 3, B = 65: 780 noise counters = three workgroups and 12 threads of a fourth; 195 positions end inside the first."""
    N, B, length, pad = 3, 65, 70, 256
    sizes = (N * B, N * B * N * 2, N * B * 2)
    raw = [torch.full((n + pad,), -12345, dtype=torch.int64, device=DEV) if k == 0 else torch.full((n + pad,), -12345.0, dtype=torch.float32, device=DEV)
           for k, n in enumerate(sizes)]
    out = (raw[0][:sizes[0]].view(N, B), raw[1][:sizes[1]].view(N, B, N, 2), raw[2][:sizes[2]].view(N, B, 2))
    gu.maddpg_draws(N, B, length, SEED, STEP, DEV, out=out)
    assert np.array_equal(out[0].cpu().numpy(), dr.index(N, B, length, SEED, STEP))
    _check_noise(out[1], out[2], N, B, SEED, STEP)
    for buf, n in zip(raw, sizes):
        assert bool((buf[n:] == -12345).all())


def test_wrapper_refusals():
    with pytest.raises(ValueError, match="distinct"):
        gu.maddpg_draws(3, 11, 10, SEED, STEP, DEV)
    with pytest.raises(ValueError):
        gu.maddpg_draws(0, 4, 10, SEED, STEP, DEV)
    with pytest.raises(ValueError, match="out"):
        gu.maddpg_draws(3, 4, 10, SEED, STEP, DEV, out=(torch.zeros((3, 4), dtype=torch.int32, device=DEV),) * 3)
