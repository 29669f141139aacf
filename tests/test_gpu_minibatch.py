"""csrc/mdr_minibatch.hip and mdr_adam_step_table on the GPU: the permutation and the sampled positions equal the numpy restatement
of tests/minibatch_ref.py integer for integer, the cursor kernels write what they are told and nothing else, and the Adam step with
its bias corrections read from device memory gives mdr_adam_step's bits in both launch forms."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from mdr_amd import graph_update as gu
from mdr_amd import optim
from tests import minibatch_ref as mr
from tests import optim_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xFEDCBA9876543210
BIG_EPOCH = (3 << 32) | 17      # above 2^32: the high word goes into counter word 3


def _i32(values):
    return torch.tensor([gu._i32(v) for v in values], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 4097, 70001])
def test_permutation_equals_the_restatement(n):
    for epoch in (0, 6, BIG_EPOCH):
        want = mr.permutation(n, SEED, epoch)
        assert np.array_equal(gu.permutation(n, SEED, epoch, DEV).cpu().numpy(), want), epoch
    # the cursor: a device int32 added to the low word of the epoch, with the key from the host and from the device
    cursor, key = _i32([4]), _i32([SEED & 0xFFFFFFFF, SEED >> 32])
    want = mr.permutation(n, SEED, BIG_EPOCH + 4)
    assert np.array_equal(mr.permutation(n, SEED, BIG_EPOCH, cursor=4), want)
    assert np.array_equal(gu.permutation(n, SEED, BIG_EPOCH, DEV, cursor=cursor).cpu().numpy(), want)
    assert np.array_equal(gu.permutation(n, 0, BIG_EPOCH, DEV, cursor=cursor, key=key).cpu().numpy(), want)
    # into a caller's buffer: n elements, the guard words behind them untouched
    out = torch.full((n + 4,), -7, dtype=torch.int64, device=DEV)
    got = gu.permutation(n, SEED, 6, DEV, out=out)
    assert np.array_equal(got.cpu().numpy(), mr.permutation(n, SEED, 6)) and bool((out[n:] == -7).all())


def test_permutation_of_nothing_launches_nothing():
    assert gu.permutation(0, SEED, 0, DEV).numel() == 0
    with pytest.raises(ValueError):
        gu.permutation(-1, SEED, 0, DEV)


@pytest.mark.parametrize("nb,length", [(1, 1), (256, 256), (256, 257), (1000, 524288)])
def test_sample_equals_the_restatement(nb, length):
    step = (5 << 32) | 123
    want = mr.sample(nb, length, SEED, step)
    assert want.max() < length
    host = gu.sample(nb, length, SEED, step, DEV).cpu().numpy()
    dev_len = torch.tensor([length], dtype=torch.int64, device=DEV)
    dev = gu.sample(nb, dev_len, SEED, step, DEV).cpu().numpy()
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert host.min() >= 0 and host.max() < length
    cursor, key = _i32([9]), _i32([SEED & 0xFFFFFFFF, SEED >> 32])
    out = torch.full((nb + 4,), -7, dtype=torch.int64, device=DEV)
    got = gu.sample(nb, dev_len, 0, step, DEV, out=out, cursor=cursor, key=key)
    assert np.array_equal(got.cpu().numpy(), mr.sample(nb, length, SEED, step + 9)) and bool((out[nb:] == -7).all())


def test_cursor_kernels_write_what_they_are_told_and_nothing_else():
    guard = 0x5A5A5A5A
    block = torch.full((12,), guard, dtype=torch.int32, device=DEV)
    inner = block[4:8]
    gu.cursor_set(inner, [1, -2, 0x7FFFFFFF, 0xFFFFFFFF])
    assert block.cpu().tolist() == [guard] * 4 + [1, -2, 0x7FFFFFFF, -1] + [guard] * 4
    gu.cursor_set(inner, [11, 12])      # two values: the other two stay
    assert block.cpu().tolist() == [guard] * 4 + [11, 12, 0x7FFFFFFF, -1] + [guard] * 4
    gu.cursor_set(inner, [5], offset=3)
    gu.cursor_add(inner, 0, 4)
    gu.cursor_add(inner, 1, -20)
    gu.cursor_add(inner, 0, 1)
    assert block.cpu().tolist() == [guard] * 4 + [16, -8, 0x7FFFFFFF, 5] + [guard] * 4
    for bad in (lambda: gu.cursor_set(inner, []), lambda: gu.cursor_set(inner, [1] * 5), lambda: gu.cursor_set(inner, [1, 2], offset=3),
                lambda: gu.cursor_add(inner, 4, 1)):
        with pytest.raises(ValueError):
            bad()
    assert block.cpu().tolist() == [guard] * 4 + [16, -8, 0x7FFFFFFF, 5] + [guard] * 4


# -- mdr_adam_step_table against mdr_adam_step ------------------------------------------------------------------------------------------
LR, MAX_NORM, CLAMP, TAU = 1e-3, 0.5, 0.5, 0.01
MODES = {"clip": dict(max_grad_norm=MAX_NORM), "clamp-blend": dict(grad_clamp=CLAMP, blend=True), "neither": dict()}


class _Net:
    """Parameters, targets and a FusedAdam over them, the gradients slices of one flat buffer (odd float offsets)."""

    def __init__(self, shapes, max_fused_floats):
        self.p = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in ref.draw(shapes, 1)]
        self.target = [torch.from_numpy(x).to(DEV) for x in ref.draw(shapes, 2)]
        self.opt = optim.FusedAdam(self.p, LR, max_fused_floats=max_fused_floats)
        self.buf = torch.zeros(sum(p.numel() for p in self.p), dtype=torch.float32, device=DEV)
        off = 0
        for p in self.p:
            p.grad = self.buf[off:off + p.numel()].view_as(p)
            off += p.numel()

    def set_grad(self, g):
        for p, x in zip(self.p, g):
            p.grad.copy_(torch.from_numpy(x))

    def bits(self, norm):
        out = [t.detach().cpu().numpy().copy() for t in self.p + self.target + [self.opt._exp_avg, self.opt._exp_avg_sq]]
        return out + [None if norm is None else norm.cpu().numpy().copy()]


@pytest.mark.parametrize("fused", [1, 0], ids=["two-launches", "library-default"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["ones", "six", "ragged"])
def test_table_step_gives_the_step_count_paths_bits(name, mode, fused):
    """Four steps from step 7 on: the plain call at steps 7..10 against the table call reading pairs 0 and 3 (the first and the last
    slot) directly and pairs 1 and 2 through base_dev; p, m, v, target and total_norm bit for bit, the host's counts untouched until
    advance()."""
    shapes, kw = ref.CASES[name], dict(MODES[mode])
    blend = kw.pop("blend", False)
    want_norm = mode != "neither"
    plain, table = _Net(shapes, fused), _Net(shapes, fused)
    if name == "six":
        assert plain.p[1].grad.data_ptr() % 16 != 0      # the first bias at float 35 of the flat gradient
    for net in (plain, table):      # six steps first: nonzero moments, step count 6
        for t in range(1, 7):
            net.set_grad(ref.draw(shapes, 50 + t, 1.0))
            net.opt.step(max_grad_norm=MAX_NORM)
    corrections = table.opt.correction_table(4).to(DEV)
    assert table.opt.step_count() == 6
    base = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k, (slot, b) in enumerate(((0, None), (0, 1), (1, 1), (3, None))):
        g = ref.draw(shapes, 100 + k, 3.0 if k % 2 == 0 else 0.001)      # clipped and unclipped
        extra = dict(target=plain.target, tau=TAU) if blend else {}
        plain.set_grad(g)
        norm = plain.opt.step(want_norm=want_norm, **kw, **extra)
        want = plain.bits(norm)
        extra = dict(target=table.target, tau=TAU) if blend else {}
        table.set_grad(g)
        if b is not None:
            base.fill_(b)
        norm = table.opt.step(want_norm=want_norm, **kw, **extra, corrections=corrections, slot=slot, base_dev=base if b is not None else None)
        got = table.bits(norm)
        for x, y in zip(got, want):
            assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), (k, slot, b)
        assert table.opt.step_count() == 6 and table.opt._t == 6
    table.opt.advance(4)
    assert table.opt.step_count() == plain.opt.step_count() == 10 and table.opt._t == plain.opt._t == 10
    assert all(float(table.opt.state[p]["step"]) == 10.0 for p in table.p)


def test_table_step_keywords_are_checked():
    net = _Net(ref.CASES["six"], 0)
    net.set_grad(ref.draw(ref.CASES["six"], 3))
    corrections = net.opt.correction_table(2).to(DEV)
    before = [p.detach().clone() for p in net.p]
    for kw in (dict(slot=0), dict(corrections=corrections), dict(corrections=corrections, slot=2), dict(corrections=corrections, slot=-1),
               dict(corrections=corrections.cpu(), slot=0), dict(corrections=corrections[:3], slot=0),
               dict(corrections=corrections, slot=0, base_dev=torch.zeros(1, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            net.opt.step(**kw)
    assert all(torch.equal(a, b) for a, b in zip(before, net.p)) and net.opt.step_count() == 0
