"""The wide entry points (include/mdr_policy.h: mdr_*_wide, 65..128 input features) on the GPU, against the fp64 restatements and the
derived rounding bounds of tests/ppo_grad_ref.py, tests/dqn_grad_ref.py and tests/mappo_grad_ref.py: every element of every output
at worst |error| / bound <= 1, next_action exactly.  The harnesses are those of the narrow entry points' tests
(tests/test_gpu_ppo_grad.py, test_gpu_dqn_grad.py, test_gpu_mappo_grad.py) with each C symbol replaced by its wide sibling, which has
the same argument list; tests/test_wide_grad.py shows on the CPU that the bounds mean at these widths what they mean at 51."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import dqn_grad_ref as dr
from tests import mappo_grad_ref as mr
from tests import ppo_grad_ref as pr
from tests import test_gpu_dqn_grad as dg
from tests import test_gpu_mappo_grad as mg
from tests import test_gpu_ppo_grad as pg
from tests.test_wide_grad import JOINT_SHAPES, JOINT_SWEEP, MAIN, NARROW, SWEEP, WIDE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_dev, _ptr = pg._dev, pg._ptr


class _WideLib:
    """The library with every narrow name answered by its wide sibling."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, WIDE.get(name, name))


def _wide(cls):
    class Wide(cls):
        def __init__(self, *args, **kwargs):
            lib = _WideLib(nat.load())
            with mock.patch.object(nat, "load", lambda: lib):      # the harness takes its library from nat.load() while it is built
                super().__init__(*args, **kwargs)
            assert isinstance(self.lib, _WideLib)
    Wide.__name__ = "Wide" + cls.__name__
    return Wide


PPOCall, DQNCall, JointCall = _wide(pg.Call), _wide(dg.Call), _wide(mg.Call)
JOINT_MAIN = JOINT_SHAPES[2]      # (121, 8, 100, 100): 128 joint inputs
KINDS = ["actor", "critic", "dqn", "ddqn", "joint"]


def _reference(kind, B, net=None):
    if kind in ("actor", "critic"):
        return pr.reference(B, *(net or MAIN), 2 if kind == "actor" else 1)
    if kind in ("dqn", "ddqn"):
        return dr.reference(B, *(net or MAIN), kind == "ddqn")
    return mr.reference(B, *(net or JOINT_MAIN))


def _call(kind, d, net=None, **kw):
    if kind in ("actor", "critic"):
        return PPOCall(d, 2 if kind == "actor" else 1, **kw)
    if kind in ("dqn", "ddqn"):
        return DQNCall(d, kind == "ddqn", **kw)
    return JointCall(d, (net or JOINT_MAIN)[1], **kw)


def _check(kind, got, r, label):
    {"actor": pg._check, "critic": pg._check, "dqn": dg._check, "ddqn": dg._check, "joint": mg._check}[kind](got, r, kind + " " + label)


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=False), k


# ---- the sweep within the derived bound

@pytest.mark.parametrize("kind", KINDS[:4])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B%d-F%d-H%d-%d" % c)
def test_sweep_matches_fp64_within_the_bound(case, kind):
    r = _reference(kind, case[0], case[1:])
    call = _call(kind, r["inputs"])
    assert call.run() == nat.MDR_OK
    _check(kind, call.results(), r, "B%d F%d H%d/%d" % case)


@pytest.mark.parametrize("case", JOINT_SWEEP, ids=lambda c: "B%d-F%d-N%d-H%d-%d" % c)
def test_joint_sweep_matches_fp64_within_the_bound(case):
    r = mr.reference(*case)
    call = JointCall(r["inputs"], case[2])
    assert call.M >= call.B and call.M % case[2] == 0 and call.net.num_state > 100
    assert call.run() == nat.MDR_OK
    _check("joint", call.results(), r, "B%d F%d N%d H%d/%d" % case)


# ---- grid shapes

@pytest.mark.parametrize("kind", KINDS)
def test_two_workgroups_take_several_tiles_and_a_partial_one(kind):
    B = 16 * 7 + 5      # 8 tiles over 2 workgroups: four each, the last one of 5 rows
    r = _reference(kind, B)
    call = _call(kind, r["inputs"], max_workgroups=2)
    assert call.run() == nat.MDR_OK
    _check(kind, call.results(), r, "max_workgroups=2")


@pytest.mark.parametrize("kind", KINDS)
def test_one_row_beyond_a_full_pass_of_the_library_grid(kind):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * min(cus, 512) + 1
    assert B < 10 ** 5
    r = _reference(kind, B)
    call = _call(kind, r["inputs"])
    assert call.run() == nat.MDR_OK
    _check(kind, call.results(), r, "B%d own grid" % B)


@pytest.mark.parametrize("kind", KINDS[:4])
def test_index_equals_the_gathered_copy_bit_for_bit(kind):
    M, B = 257, 100
    d = _reference(kind, M)["inputs"]
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [200, 3, 200, 3]      # repeats, out of order
    gathered = dict(d, **{k: d[k][idx] for k in ("x", "xn", "action", "old", "target", "reward") if k in d})
    if kind == "actor":      # the advantage is in minibatch order
        d, gathered = dict(d, adv=d["adv"][:B]), dict(gathered, adv=d["adv"][:B])
    a, b = _call(kind, d, index=_dev(idx.astype(np.int64))), _call(kind, gathered)
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    _same_bits(a.results(), b.results())
    if kind in ("dqn", "ddqn"):
        r = dict(ref=dr.evaluate(gathered, double=kind == "ddqn"), bound=dr.bound(gathered, kind == "ddqn"))
    else:
        r = dict(ref=pr.evaluate(gathered), bound=pr.bound(gathered))
    _check(kind, b.results(), r, "gathered")


def test_joint_index_equals_the_gathered_copy_bit_for_bit():
    F, N, H1, H2 = JOINT_MAIN
    M, B = 33 * N, 100
    full = mr.case(M, F, N, H1, H2, M=M)["inputs"]      # x: the joint rows of the whole buffer
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:8] = [M - 1, 0, N - 1, M - N, M - 1, 0, 200, 3]      # agent 0 and agent N - 1 of the first and the last env; repeats, out of order
    group = (idx - idx % N)[:, None] + np.arange(N)[None, :]      # minibatch row i's whole env group at rows i N .. i N + N - 1
    gathered = dict(full, state=full["state"][group.reshape(-1)], action=full["action"][group.reshape(-1)],
                    buffer_target=full["buffer_target"][group.reshape(-1)])
    a = JointCall(full, N, index=_dev(idx.astype(np.int64)))
    b = JointCall(gathered, N, index=_dev((np.arange(B) * N + idx % N).astype(np.int64)))
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    _same_bits(a.results(), b.results())
    d = dict(full, x=full["x"][idx], target=full["buffer_target"][idx])
    _check("joint", a.results(), dict(ref=pr.evaluate(d), bound=pr.bound(d)), "index")


@pytest.mark.parametrize("kind", KINDS)
def test_strided_states_and_canaries(kind):
    """State rows of 121 floats inside rows of 160, NaN between the rows and in a whole row behind the last; NaN on either side of
    every output."""
    B, LD = 65, 160
    r = _reference(kind, B)
    d = r["inputs"]
    F = MAIN[0]
    rows = d["state"] if kind == "joint" else d["x"]
    M = rows.shape[0]
    images = {}
    for k, src in (("state", rows),) + ((("next_state", d["xn"]),) if kind in ("dqn", "ddqn") else ()):
        buf = torch.full((M + 1, LD), NAN, dtype=torch.float32, device=DEV)
        buf[:M, 7:7 + F] = _dev(src)
        images[k] = buf[:M, 7:7 + F]
    call = _call(kind, d, ld=LD, pad=64, **images)
    assert call.run() == nat.MDR_OK
    assert call.canaries_intact()
    _check(kind, call.results(), r, "ld_state=%d" % LD)


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_equal_bits(kind):
    r = _reference(kind, 257)
    call = _call(kind, r["inputs"], max_workgroups=3)
    assert call.run() == nat.MDR_OK
    first = call.results()
    assert call.run() == nat.MDR_OK
    _same_bits(first, call.results())


def test_zero_rows_write_zeros():
    for kind in ("actor", "critic", "joint"):
        call = _call(kind, _reference(kind, 16)["inputs"])
        assert call.run(B=0) == nat.MDR_OK
        assert bool((call.out("grad") == 0).all()) and float(call.out("loss")[0]) == 0.0, kind
    call = _call("ddqn", _reference("ddqn", 16)["inputs"])
    assert call.run_target(B=0) == nat.MDR_OK and call.untouched(("y", "next_q", "next_action"))
    assert call.run_grad(B=0) == nat.MDR_OK
    assert bool((call.out("grad") == 0).all()) and float(call.out("loss")[0]) == 0.0


# the wide limits: 128 inputs, 128 hidden units, the LDS fit (128-128 holds 100 inputs)
SHAPES_REFUSED = (dict(num_state=129), dict(hidden1=129), dict(hidden2=129), dict(num_state=101, hidden1=128, hidden2=128))


@pytest.mark.parametrize("O", [2, 1], ids=["actor", "critic"])
def test_ppo_refusals_leave_the_outputs_untouched(O):
    call = PPOCall(pr.inputs(33, *MAIN, O), O)
    invalid = [dict(net=None), dict(state=None), dict(grad=None), dict(loss=None), dict(ws=None), dict(w0=None), dict(ld=120), dict(B=-1),
               dict(mw=-1), dict(ws=C.c_void_p(call.ws.data_ptr() + 4))]
    if O == 2:
        invalid += [dict(w1=None), dict(adv=None), dict(clip=C.c_float(-0.1)), dict(clip=C.c_float(1.0)), dict(clip=C.c_float(NAN))]
    for ov in invalid:
        assert call.run(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(), ov
    assert call.run(net=dg._wrong(call.net, struct_size=call.net.struct_size - 8)) == nat.MDR_ERR_INVALID and call.untouched()
    for fields in SHAPES_REFUSED + (dict(num_out=3 - O), dict(num_out=3)):
        assert call.run(net=dg._wrong(call.net, **fields), ld=256) == nat.MDR_ERR_UNSUPPORTED, fields      # ld_state >= F: the shape alone
        assert call.untouched(), fields
    torch.cuda.synchronize()


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
def test_dqn_refusals_leave_the_outputs_untouched(double):
    call = DQNCall(dr.inputs(33, *MAIN), double)
    outs = ("y", "next_q", "next_action")
    invalid = [dict(target=None), dict(next_state=None), dict(reward=None), dict(y=None), dict(ld=120), dict(B=-1), dict(mw=-1),
               dict(gamma=C.c_float(NAN)), dict(target=dg._wrong(call.target, struct_size=8))]
    if double:
        invalid += [dict(next_action=None), dict(policy=dg._wrong(call.policy, struct_size=8)), dict(policy=dg._wrong(call.policy, w2=None))]
    for ov in invalid:
        assert call.run_target(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(outs), ov
    unsupported = [dict(target=dg._wrong(call.target, **f), ld=256) for f in SHAPES_REFUSED + (dict(num_out=1), dict(num_out=3))]
    if double:      # two nets of different shapes
        unsupported += [dict(policy=dg._wrong(call.policy, **{f: v})) for f, v in (("num_state", 120), ("hidden1", 96), ("hidden2", 96))]
    for ov in unsupported:
        assert call.run_target(**ov) == nat.MDR_ERR_UNSUPPORTED, ov
        assert call.untouched(outs), ov
    assert call.run_target() == nat.MDR_OK
    y = call.out("y").clone()
    outs = ("grad", "loss", "q")
    for ov in (dict(net=None), dict(state=None), dict(grad=None), dict(loss=None), dict(ws=None), dict(action=None), dict(y_in=None), dict(ld=120),
               dict(B=-1), dict(mw=-1), dict(ws=C.c_void_p(call.ws.data_ptr() + 4)), dict(clamp=C.c_float(0.0)), dict(clamp=C.c_float(NAN)),
               dict(net=dg._wrong(call.policy, struct_size=8))):
        assert call.run_grad(y=y, **ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(outs), ov
    for fields in SHAPES_REFUSED + (dict(num_out=1), dict(num_out=3)):
        assert call.run_grad(y=y, net=dg._wrong(call.policy, **fields), ld=256) == nat.MDR_ERR_UNSUPPORTED, fields
        assert call.untouched(outs), fields
    torch.cuda.synchronize()


def test_joint_refusals_leave_the_outputs_untouched():
    F, N = JOINT_MAIN[:2]
    call = JointCall(mr.reference(33, *JOINT_MAIN)["inputs"], N)
    invalid = [dict(net=None), dict(state=None), dict(action=None), dict(target=None), dict(grad=None), dict(loss=None), dict(ws=None),
               dict(N=0), dict(N=-1), dict(N=F + N), dict(ld=F - 1), dict(M=call.M + 1), dict(M=call.M - 1), dict(B=-1), dict(mw=-1),
               dict(ws=C.c_void_p(call.ws.data_ptr() + 4)), dict(net=dg._wrong(call.net, struct_size=8))]
    for ov in invalid:
        assert call.run(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(), ov
    # the shape alone is refused: M = 0 is a multiple of every nb_agents; 140 inputs are 121 features with the reference's 20 agents
    for fields, agents in ((dict(num_out=2), N), (dict(num_state=129), 9), (dict(num_state=140), 20), (dict(hidden1=129), N),
                           (dict(hidden2=129), N), (dict(num_state=101, hidden1=128, hidden2=128), N)):
        assert call.run(net=dg._wrong(call.net, **fields), N=agents, M=0, ld=256) == nat.MDR_ERR_UNSUPPORTED, fields
        assert call.untouched(), fields
    torch.cuda.synchronize()


# ---- up to 64 features a wide entry point returns its narrow sibling's bits

@pytest.mark.parametrize("net", NARROW, ids=lambda n: "F%d-H%d-%d" % n)
@pytest.mark.parametrize("kind", KINDS[:4])
def test_wide_entry_points_return_the_narrow_ones_bits(kind, net):
    d = _reference(kind, 257, net)["inputs"]
    if kind in ("actor", "critic"):
        narrow, wide = pg.Call(d, 2 if kind == "actor" else 1, max_workgroups=3), _call(kind, d, max_workgroups=3)
    else:
        narrow, wide = dg.Call(d, kind == "ddqn", max_workgroups=3), _call(kind, d, max_workgroups=3)
    assert wide.G == narrow.G and wide.ws.numel() == narrow.ws.numel()
    assert narrow.run() == nat.MDR_OK and wide.run() == nat.MDR_OK
    _same_bits(narrow.results(), wide.results())


@pytest.mark.parametrize("shape", [(51, 20, 100, 100), (51, 14, 128, 128), (64, 65, 64, 64)], ids=lambda s: "F%d-N%d-H%d-%d" % s)
def test_wide_joint_entry_point_returns_the_narrow_one_s_bits(shape):
    """The same kernel on the two LDS layouts, at the reference's shape, at 128-128 (64 joint inputs) and at 128 joint inputs."""
    d = mr.reference(257, *shape)["inputs"]
    narrow, wide = mg.Call(d, shape[1], max_workgroups=3), JointCall(d, shape[1], max_workgroups=3)
    assert wide.G == narrow.G and wide.ws.numel() == narrow.ws.numel()
    assert narrow.run() == nat.MDR_OK and wide.run() == nat.MDR_OK
    _same_bits(narrow.results(), wide.results())
