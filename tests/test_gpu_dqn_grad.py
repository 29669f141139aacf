"""mdr_dqn_target / mdr_dqn_grad (include/mdr_policy.h) and mdr_amd.dqn's two calls on the GPU, against the fp64 restatement and the
derived rounding bound of tests/dqn_grad_ref.py: every element of y, next_q, q, loss and grad at worst |error| / bound <= 1,
next_action exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import dqn_grad_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")
FLOAT_OUTS = ("y", "next_q", "q", "loss", "grad")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Call:
    """The two C calls of one update on device copies of a case's inputs; every output and the workspace NaN-filled (next_action:
    0xEE) before each."""

    def __init__(self, d, double=False, max_workgroups=0, index=None, state=None, next_state=None, ld=None, pad=0):
        self.lib = nat.load()
        self.double, self.mw, self.clamp = double, max_workgroups, float(d["clamp"])
        H1, F = d["W1"].shape
        H2 = d["W2"].shape[0]
        self.params = [_dev(d[k]) for k in dr.PARAM_NAMES]
        self.tparams = [_dev(d[k]) for k in dr.TARGET_NAMES]
        self.policy = nat.MdrMlp(C.sizeof(nat.MdrMlp), F, H1, H2, 2, *[_ptr(p) for p in self.params])
        self.target = nat.MdrMlp(C.sizeof(nat.MdrMlp), F, H1, H2, 2, *[_ptr(p) for p in self.tparams])
        self.state = _dev(d["x"]) if state is None else state
        self.next_state = _dev(d["xn"]) if next_state is None else next_state
        self.ld = F if ld is None else ld
        self.index = index
        self.B = int(index.shape[0]) if index is not None else int(d["x"].shape[0])
        self.action, self.reward = _dev(d["action"]), _dev(d["reward"])
        self.G = int(self.lib.mdr_mlp_grad_floats(C.byref(self.policy)))
        nbytes = int(self.lib.mdr_mlp_grad_workspace_bytes(C.byref(self.policy), self.B, max_workgroups))
        assert self.G > 0 and nbytes > 0
        self.pad = pad      # canary elements on either side of every output
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        self.bufs = {k: torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV)
                     for k, n in (("grad", self.G), ("loss", 1), ("y", self.B), ("next_q", self.B), ("q", self.B))}
        self.bufs["next_action"] = torch.empty(self.B + 2 * pad, dtype=torch.uint8, device=DEV)

    def out(self, k):
        b = self.bufs[k]
        return b[self.pad:b.numel() - self.pad]

    def _fill(self, keys):
        for k in keys:
            self.bufs[k].fill_(0xEE if k == "next_action" else NAN)

    def run_target(self, **override):
        self._fill(("y", "next_q", "next_action"))
        a = dict(target=C.byref(self.target), policy=C.byref(self.policy) if self.double else None, next_state=_ptr(self.next_state),
                 ld=self.ld, index=_ptr(self.index), B=self.B, reward=_ptr(self.reward), gamma=C.c_float(dr.GAMMA), mw=self.mw,
                 y=_ptr(self.out("y")), next_q=_ptr(self.out("next_q")), next_action=_ptr(self.out("next_action")))
        a.update(override)
        return self.lib.mdr_dqn_target(a["target"], a["policy"], a["next_state"], a["ld"], a["index"], a["B"], a["reward"], a["gamma"], a["mw"],
                                       a["y"], a["next_q"], a["next_action"], C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run_grad(self, y=None, **override):
        """`y`: the device tensor the gradient call reads (default: what run_target left)."""
        y_in = self.out("y").clone() if y is None else y
        self.ws.fill_(NAN)
        self._fill(("grad", "loss", "q"))
        a = dict(net=C.byref(self.policy), state=_ptr(self.state), ld=self.ld, index=_ptr(self.index), B=self.B, action=_ptr(self.action),
                 y_in=_ptr(y_in), clamp=C.c_float(self.clamp), mw=self.mw, ws=_ptr(self.ws), grad=_ptr(self.out("grad")),
                 loss=_ptr(self.out("loss")), q=_ptr(self.out("q")))
        a.update(override)
        return self.lib.mdr_dqn_grad(a["net"], a["state"], a["ld"], a["index"], a["B"], a["action"], a["y_in"], a["clamp"], a["mw"], a["ws"],
                                     a["grad"], a["loss"], a["q"], C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self):
        rc = self.run_target()
        return rc if rc != nat.MDR_OK else self.run_grad()

    def results(self):
        r = {k: self.out(k).cpu().numpy() for k in ("y", "next_q", "q", "grad", "next_action")}
        r["loss"] = self.out("loss").cpu().numpy()[0]
        return r

    def untouched(self, keys):
        return all(bool(torch.isnan(self.bufs[k]).all()) if k != "next_action" else bool((self.bufs[k] == 0xEE).all()) for k in keys)

    def canaries_intact(self):
        p = self.pad
        ok = True
        for k, b in self.bufs.items():
            edge = torch.cat([b[:p], b[b.numel() - p:]])
            ok &= bool((edge == 0xEE).all()) if k == "next_action" else bool(torch.isnan(edge).all())
        return ok


def _check(got, r, label):
    assert np.array_equal(got["next_action"], r["ref"]["next_action"]), label
    for k in FLOAT_OUTS:
        w = dr.worst(got[k], r["ref"][k], r["bound"][k])
        print("%s %-7s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


MODES = pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])


@MODES
@pytest.mark.parametrize("case", dr.SWEEP, ids=lambda c: "B%d-F%d-H%d-%d" % c)
def test_sweep_matches_fp64_within_the_bound(case, double):
    r = dr.reference(*case, double)
    call = Call(r["inputs"], double)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "B%d F%d H%d/%d %s" % (case + ("ddqn" if double else "dqn",)))


@MODES
def test_two_workgroups_take_several_tiles_and_a_partial_one(double):
    B = 16 * 7 + 5      # 8 tiles over 2 workgroups: four each, the last one of 5 rows
    r = dr.reference(B, 51, 100, 100, double)
    call = Call(r["inputs"], double, max_workgroups=2)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "max_workgroups=2")


@MODES
def test_one_row_beyond_a_full_pass_of_the_library_grid(double):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * min(cus, 512) + 1
    assert B < 10 ** 5
    d = dr.inputs(B, 51, 100, 100)
    r = dict(inputs=d, ref=dr.evaluate(d, double=double), bound=dr.bound(d, double))
    call = Call(d, double)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "B%d own grid" % B)


@MODES
def test_index_equals_the_gathered_copy_bit_for_bit(double):
    M, B = 257, 100
    d = dr.inputs(M, 51, 100, 100)
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [200, 3, 200, 3]      # repeats, out of order
    gathered = dict(d, **{k: d[k][idx] for k in dr.ROW_KEYS})
    a, b = Call(d, double, index=_dev(idx.astype(np.int64))), Call(gathered, double)
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    _check(rb, dict(ref=dr.evaluate(gathered, double=double), bound=dr.bound(gathered, double)), "gathered")


@MODES
def test_strided_states_and_canaries(double):
    B, F = 65, 51
    r = dr.reference(B, F, 100, 100, double)
    wide = torch.full((2, B, 80), NAN, dtype=torch.float32, device=DEV)
    wide[0, :, 7:7 + F] = _dev(r["inputs"]["x"])
    wide[1, :, 7:7 + F] = _dev(r["inputs"]["xn"])
    call = Call(r["inputs"], double, state=wide[0, :, 7:7 + F], next_state=wide[1, :, 7:7 + F], ld=80, pad=64)
    assert call.run() == nat.MDR_OK
    assert call.canaries_intact()
    _check(call.results(), r, "ld_state=80")


@MODES
def test_two_calls_give_equal_bits(double):
    r = dr.reference(257, 51, 100, 100, double)
    call = Call(r["inputs"], double, max_workgroups=3)
    assert call.run() == nat.MDR_OK
    first = call.results()
    assert call.run() == nat.MDR_OK
    second = call.results()
    for k in first:
        assert np.array_equal(first[k], second[k]), k


@MODES
def test_clamp_at_the_median_gradient(double):
    r = dr.reference(257, 51, 100, 100, double, "median")
    c = r["inputs"]["clamp"]
    clamped = float((np.abs(r["ref"]["grad"]) == c).mean())
    assert 0.25 <= clamped <= 0.75, clamped
    call = Call(r["inputs"], double)
    assert call.run() == nat.MDR_OK
    got = call.results()
    assert float(np.abs(got["grad"]).max()) == float(np.float32(c))
    _check(got, r, "clamp %.3g" % c)


def test_infinite_clamp_equals_a_clamp_beyond_every_element():
    d = dr.inputs(257, 51, 100, 100)
    call = Call(d)
    assert call.clamp == INF and call.run() == nat.MDR_OK
    free = call.results()
    big = float(np.abs(free["grad"]).max()) * 2
    call.clamp = big
    assert call.run() == nat.MDR_OK
    limited = call.results()
    assert np.array_equal(free["grad"], limited["grad"]) and free["loss"] == limited["loss"]


@pytest.mark.parametrize("clamp", [INF, 1.0, 1e-3])
def test_nan_in_y_stays_nan_through_the_clamp(clamp):
    """clamp_ keeps a NaN; fminf / fmaxf would turn it into the bound."""
    d = dict(dr.inputs(33, 51, 100, 100), clamp=clamp)
    call = Call(d)
    assert call.run_target() == nat.MDR_OK
    y = call.out("y").clone()
    y[17] = NAN
    assert call.run_grad(y=y) == nat.MDR_OK
    got = call.results()
    s = dr.param_slices(51, 100, 100, 2)
    a = int(d["action"][17])
    assert np.isnan(got["loss"]) and np.isnan(got["grad"][s["b3"]][a]) and not np.isnan(got["grad"][s["b3"]][1 - a])
    assert np.isnan(got["grad"][s["W3"]].reshape(2, -1)[a]).all()
    assert np.isnan(got["q"]).sum() == 0


def test_zero_rows_write_zeros():
    d = dr.inputs(16, 51, 100, 100)
    call = Call(d)
    assert call.run_target(B=0) == nat.MDR_OK and call.untouched(("y", "next_q", "next_action"))
    assert call.run_grad(B=0) == nat.MDR_OK
    assert bool((call.out("grad") == 0).all()) and float(call.out("loss")[0]) == 0.0


def _wrong(net, **fields):
    twin = nat.MdrMlp.from_buffer_copy(net)
    for k, v in fields.items():
        setattr(twin, k, v)
    return C.byref(twin)


def test_refusals_of_the_gradient_call_leave_the_outputs_untouched():
    call = Call(dr.inputs(33, 51, 100, 100))
    assert call.run_target() == nat.MDR_OK
    y = call.out("y").clone()
    outs = ("grad", "loss", "q")
    invalid = [dict(net=None), dict(state=None), dict(grad=None), dict(loss=None), dict(ws=None), dict(action=None), dict(y_in=None), dict(ld=50),
               dict(B=-1), dict(mw=-1), dict(ws=C.c_void_p(call.ws.data_ptr() + 4)), dict(clamp=C.c_float(0.0)), dict(clamp=C.c_float(-1.0)),
               dict(clamp=C.c_float(NAN)), dict(net=_wrong(call.policy, struct_size=call.policy.struct_size - 8))]
    for ov in invalid:
        assert call.run_grad(y=y, **ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(outs), ov
    for field, value in (("num_state", 65), ("hidden1", 129), ("hidden2", 129), ("num_out", 1), ("num_out", 3)):
        assert call.run_grad(y=y, net=_wrong(call.policy, **{field: value}), ld=128) == nat.MDR_ERR_UNSUPPORTED, (field, value)
        assert call.untouched(outs), (field, value)
    torch.cuda.synchronize()


@MODES
def test_refusals_of_the_target_call_leave_the_outputs_untouched(double):
    call = Call(dr.inputs(33, 51, 100, 100), double)
    outs = ("y", "next_q", "next_action")
    invalid = [dict(target=None), dict(next_state=None), dict(reward=None), dict(y=None), dict(ld=50), dict(B=-1), dict(mw=-1),
               dict(gamma=C.c_float(NAN)), dict(gamma=C.c_float(INF)), dict(target=_wrong(call.target, struct_size=call.target.struct_size - 8))]
    if double:
        invalid += [dict(next_action=None), dict(policy=_wrong(call.policy, struct_size=8)), dict(policy=_wrong(call.policy, w2=None))]
    for ov in invalid:
        assert call.run_target(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(outs), ov
    unsupported = [dict(target=_wrong(call.target, **{f: v}), ld=128)
                   for f, v in (("num_state", 65), ("hidden1", 129), ("hidden2", 129), ("num_out", 1), ("num_out", 3))]
    if double:      # two nets of different shapes
        unsupported += [dict(policy=_wrong(call.policy, **{f: v})) for f, v in (("num_state", 50), ("hidden1", 96), ("hidden2", 96), ("num_out", 1))]
    for ov in unsupported:
        assert call.run_target(**ov) == nat.MDR_ERR_UNSUPPORTED, ov
        assert call.untouched(outs), ov
    if not double:      # DQN takes a missing next_action and next_q
        assert call.run_target(next_action=None, next_q=None) == nat.MDR_OK
        assert call.untouched(("next_q", "next_action")) and not bool(torch.isnan(call.out("y")).any())
    torch.cuda.synchronize()


def _modules(d, F, H1, H2):
    from mdr_amd.dqn import QNetworkMLP
    nets = []
    for names in (dr.PARAM_NAMES, dr.TARGET_NAMES):
        net = QNetworkMLP(F, layers=(H1, H2)).to(DEV)
        with torch.no_grad():
            for p, k in zip((t for lin in net.fc for t in (lin.weight, lin.bias)), names):
                p.copy_(_dev(d[k]))
        nets.append(net)
    return nets


@MODES
def test_python_calls_fill_grad_with_what_the_c_call_wrote(double):
    from mdr_amd import dqn
    B, F, H1, H2 = 65, 51, 100, 100
    d = dict(dr.inputs(B, F, H1, H2), clamp=1.0)
    policy, target = _modules(d, F, H1, H2)
    call = Call(d, double)
    assert call.run() == nat.MDR_OK
    want = call.results()
    y, next_q, next_action = dqn.td_target(target, _dev(d["xn"]), _dev(d["reward"]), dr.GAMMA, policy_net=policy if double else None)
    assert next_action.dtype == torch.uint8
    for k, t in (("y", y), ("next_q", next_q), ("next_action", next_action)):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    policy.fc[0].weight.grad = torch.full_like(policy.fc[0].weight, NAN)      # an existing gradient is overwritten, a missing one made
    assert policy.fc[1].weight.grad is None
    loss, q = dqn.q_loss_backward(policy, _dev(d["x"]), _dev(d["action"]), y, grad_clamp=1.0, want_q=True)
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(want["loss"])
    assert np.array_equal(q.cpu().numpy(), want["q"])
    got = torch.cat([p.grad.reshape(-1) for lin in policy.fc for p in (lin.weight, lin.bias)]).cpu().numpy()
    assert np.array_equal(got, want["grad"])


def test_supported_and_value_errors():
    from mdr_amd import dqn
    from mdr_amd.rollout import CriticMLP
    net = dqn.QNetworkMLP(51).to(DEV)
    assert dqn.supported(net)
    wide, deep, cpu, critic = dqn.QNetworkMLP(81).to(DEV), dqn.QNetworkMLP(51, layers=(100, 100, 100)).to(DEV), dqn.QNetworkMLP(51), CriticMLP(51).to(DEV)
    assert not any(dqn.supported(n) for n in (wide, deep, cpu, critic))
    x, r = torch.zeros((4, 51), device=DEV), torch.zeros(4, device=DEV)
    a = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="at most 64 input features"):
        dqn.td_target(wide, torch.zeros((4, 81), device=DEV), r, 0.99)
    with pytest.raises(ValueError, match="at most 64 input features"):
        dqn.td_target(net, x, r, 0.99, policy_net=wide)
    with pytest.raises(ValueError, match="reward"):
        dqn.td_target(net, x, r[:3], 0.99)
    with pytest.raises(ValueError, match="grad_clamp"):
        dqn.q_loss_backward(net, x, a, r, grad_clamp=0.0)
    with pytest.raises(ValueError, match="y must"):
        dqn.q_loss_backward(net, x, a, r[:3])
    with pytest.raises(ValueError, match="backend='hip'"):
        dqn.DQNLearner(wide, 1e-3, buffer_capacity=16, backend="hip")
    assert not dqn.DQNLearner(wide, 1e-3, buffer_capacity=16, backend="auto").uses_kernels(256)
    assert dqn.DQNLearner(net, 1e-3, buffer_capacity=16, backend="auto").uses_kernels(256)
