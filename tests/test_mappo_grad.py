"""The yardstick of MAPPO's joint critic kernel (tests/mappo_grad_ref.py) held to account on the CPU, and the host-only parts of the
feature: the gather's semantics, the ctypes signatures, the size helpers' answers."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import mappo_grad_ref as mr
from tests import ppo_grad_ref as pr
from tests.test_abi import _header

WRONG_SHAPES = [(51, 20, 100, 100), (51, 50, 100, 100), (8, 3, 16, 16), (63, 66, 97, 113), (51, 15, 128, 128), (64, 65, 64, 64)]


def _id(c):
    return "-".join(str(v) for v in c)


def test_others_is_the_action_dict_without_the_agent():
    """train_mappo.py:79-84 literally: copy the step's action dict, pop the agent, list(values())."""
    N, steps = 4, 3
    action = np.random.default_rng(1).integers(0, 2, steps * N)
    want = []
    for s in range(steps):
        step = {k: int(action[s * N + k]) for k in range(N)}
        for k in range(N):
            rest = dict(step)
            rest.pop(k)
            want.append(list(rest.values()))
    assert np.array_equal(mr.others(action, N), np.array(want, dtype=np.float64))
    assert mr.others(action[:N], 1 * N).shape == (N, N - 1) and mr.others(action, 1).shape == (steps * N, 0)


@pytest.mark.parametrize("T,E,N", [(3, 2, 5), (2, 4, 20), (4, 1, 2)])
def test_others_equals_the_rollout_s_others_actions(T, E, N):
    from mdr_amd.mappo import gather_others
    from mdr_amd.rollout import others_actions
    action = torch.from_numpy(np.random.default_rng([T, E, N]).integers(0, 2, (T, E * N)))
    want = others_actions(action, E, N).reshape(T * E * N, N - 1).numpy()
    assert np.array_equal(mr.others(action.numpy(), N), want.astype(np.float64))
    # the torch backend's gather of a minibatch from `action` is the same rows
    idx = torch.tensor([T * E * N - 1, 0, N - 1, N, 0])
    assert np.array_equal(gather_others(action.reshape(-1), N, idx).numpy(), want[idx.numpy()])
    assert np.array_equal(gather_others(action.reshape(-1), N).numpy(), want)


@pytest.mark.parametrize("case", mr.SWEEP, ids=_id)
def test_fp32_evaluations_stay_inside_the_bound(case):
    """z1 and z2 stay exact with the 0 / 1 action columns; an fp32 evaluation, also with every contraction permuted, is inside the
    bound on every element of every output."""
    r = mr.reference(*case)
    d = r["inputs"]
    f64, f32p = pr.forward(d, np.float64), pr.forward(d, np.float32, perm=True)
    for k in ("z1", "z2"):
        assert np.array_equal(f64[k], f32p[k].astype(np.float64)), k
    for perm in (False, True):
        got = pr.evaluate(d, np.float32, perm=perm)
        for k in r["bound"]:
            w = pr.worst(got[k], r["ref"][k], r["bound"][k])
            assert w <= 1.0, (perm, k, w)


@pytest.mark.parametrize("wrong", mr.WRONG_GATHERS)
@pytest.mark.parametrize("shape", WRONG_SHAPES, ids=_id)
def test_wrong_gathers_leave_the_bound(shape, wrong):
    """Each wrong gather puts more than half of dW1's action columns outside the bound, and the loss."""
    F, N, H1, H2 = shape
    B = 257
    r = mr.reference(B, *shape)
    d = r["inputs"]
    x = np.array(d["x"])
    x[:, F:] = mr.others(d["action"], N, wrong=wrong)[:B]
    got = pr.evaluate(mr.with_x(d, x), np.float32)
    J = F + N - 1
    ratio = pr.ratio_to_bound(got["grad"], r["ref"]["grad"], r["bound"]["grad"])[:H1 * J].reshape(H1, J)[:, F:]
    live = r["bound"]["grad"][:H1 * J].reshape(H1, J)[:, F:] > 0      # a unit that is never active has a zero gradient in both
    frac = float((ratio[live] > 1).mean())
    print("%s %s: %.3f of dW1's action columns outside the bound" % (shape, wrong, frac))
    assert frac > 0.5, frac
    assert pr.worst(got["loss"], r["ref"]["loss"], r["bound"]["loss"]) > 1.0


def _c_args(name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, _header())
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def _ctype(arg):
    if "*" in arg:
        return C.POINTER(nat.MdrMlp) if "mdr_mlp_t" in arg else C.c_void_p
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int, "float": C.c_float}[arg.split()[0]]


@pytest.mark.parametrize("name,restype", [("mdr_mappo_critic_grad_floats", C.c_int64), ("mdr_mappo_critic_workspace_bytes", C.c_int64),
                                          ("mdr_mappo_critic_grad", C.c_int)])
def test_ctypes_argtypes_match_the_header(name, restype):
    fn = getattr(nat.load(), name)
    assert name in nat.EXPORTS
    assert list(fn.argtypes) == [_ctype(a) for a in _c_args(name)]
    assert fn.restype is restype


def _net(J, H1, H2, O=1, size=None):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, J, H1, H2, O)


def test_size_helpers_answer_on_the_host():
    lib = nat.load()
    floats, nbytes = lib.mdr_mappo_critic_grad_floats, lib.mdr_mappo_critic_workspace_bytes
    G = 100 * 70 + 100 + 100 * 100 + 100 + 100 + 1
    net = _net(70, 100, 100)
    assert floats(C.byref(net), 20) == G
    stride = (G + 1 + 3) // 4 * 4 * 4
    assert nbytes(C.byref(net), 20, 33, 2) == 2 * stride            # 3 tiles of 16 rows, 2 workgroups
    assert nbytes(C.byref(net), 20, 17, 8) == 2 * stride            # never more workgroups than tiles
    assert nbytes(C.byref(net), 20, 0, 0) == stride
    assert nbytes(C.byref(net), 20, 10 ** 7, 0) == 512 * stride     # the library's own grid on any device
    assert nbytes(C.byref(net), 20, -1, 0) == -1 and nbytes(C.byref(net), 20, 16, -1) == -1
    # the required coverage fits
    assert floats(C.byref(_net(100, 112, 112)), 50) > 0 and floats(C.byref(_net(100, 100, 100)), 50) > 0
    assert floats(C.byref(_net(68, 128, 128)), 18) > 0 and floats(C.byref(_net(128, 64, 64)), 65) > 0
    assert floats(C.byref(_net(22, 100, 100)), 1) == 100 * 22 + 100 + 100 * 100 + 100 + 100 + 1
    for bad, N in (((129, 64, 64), 65), ((101, 100, 100), 51), ((69, 128, 128), 19), ((70, 129, 100), 20), ((70, 100, 129), 20),
                   ((70, 100, 100, 2), 20), ((70, 100, 100), 0), ((70, 100, 100), -3), ((70, 100, 100), 71), ((0, 100, 100), 1)):
        assert floats(C.byref(_net(*bad)), N) == -1, (bad, N)
        assert nbytes(C.byref(_net(*bad)), N, 256, 0) == -1, (bad, N)
    assert floats(C.byref(_net(70, 100, 100, size=8)), 20) == -1 and floats(None, 20) == -1
    # the PPO heads keep their own limit
    assert lib.mdr_mlp_grad_floats(C.byref(_net(70, 100, 100))) == -1
