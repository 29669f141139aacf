"""mdr_maddpg_target / mdr_maddpg_critic_grad / mdr_maddpg_actor_grad (include/mdr_policy.h) and mdr_amd.maddpg's three calls on the
GPU, against the fp64 restatement and the derived rounding bound of tests/maddpg_grad_ref.py: every element of every float output at
worst |error| / bound <= 1, next_action exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import maddpg_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
TARGET_OUTS, CRITIC_OUTS, ACTOR_OUTS = ("y", "next_q", "next_action"), ("cgrad", "closs", "q"), ("agrad", "aloss", "Q", "logits")
MID = (3, 51, 100, 100)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Call:
    """The three C calls of one agent's update on device copies of a case's inputs; every output and the workspace NaN-filled
    (next_action: 0xEE) before each."""

    def __init__(self, d, agent, tau=1.0, max_workgroups=0, index=None, state=None, next_state=None, ld=None, pad=0):
        self.lib = nat.load()
        self.agent, self.tau, self.mw = agent, tau, max_workgroups
        M, N, F = d["state"].shape
        self.N, self.F = N, F
        self.nets, self.keep = {}, []
        for prefix, O in (("", 2), ("t", 2), ("c", 1), ("tc", 1)):
            params = [_dev(d[prefix + k]) for k in R.PARAM_NAMES]
            self.keep.append(params)
            H1, K = d[prefix + "W1"].shape
            self.nets[prefix] = nat.MdrMlp(C.sizeof(nat.MdrMlp), K, H1, d[prefix + "W2"].shape[0], O, *[_ptr(p) for p in params])
        self.state = _dev(d["state"]) if state is None else state
        self.next_state = _dev(d["next_state"]) if next_state is None else next_state
        self.ld = N * F if ld is None else ld
        self.index = index
        self.B = int(index.shape[0]) if index is not None else M
        self.action, self.reward = _dev(d["action"]), _dev(d["reward"])
        # the noise is per minibatch row: with an index the caller passes the case whose noise rows are already in minibatch order
        self.noise_t = _dev(d["noise_t"][:self.B] if index is None else d["noise_t_rows"])
        self.noise_a = _dev((d["noise_a"][:self.B] if index is None else d["noise_a_rows"])[:, agent, :])
        self.Ga = int(self.lib.mdr_maddpg_grad_floats(C.byref(self.nets[""])))
        self.Gc = int(self.lib.mdr_maddpg_grad_floats(C.byref(self.nets["c"])))
        nbytes = int(self.lib.mdr_maddpg_workspace_bytes(C.byref(self.nets[""]), C.byref(self.nets["c"]), N, self.B, max_workgroups))
        assert self.Ga > 0 and self.Gc > 0 and nbytes > 0
        self.pad = pad      # canary elements on either side of every output
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        sizes = (("cgrad", self.Gc), ("closs", 1), ("agrad", self.Ga), ("aloss", 1), ("y", self.B), ("next_q", self.B), ("q", self.B), ("Q", self.B),
                 ("logits", 2 * self.B))
        self.bufs = {k: torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV) for k, n in sizes}
        self.bufs["next_action"] = torch.empty(self.B * N + 2 * pad, dtype=torch.uint8, device=DEV)

    def out(self, k):
        b = self.bufs[k]
        return b[self.pad:b.numel() - self.pad]

    def _fill(self, keys):
        for k in keys:
            self.bufs[k].fill_(0xEE if k == "next_action" else NAN)

    def run_target(self, **ov):
        self._fill(TARGET_OUTS)
        a = dict(actor=C.byref(self.nets["t"]), critic=C.byref(self.nets["tc"]), next_state=_ptr(self.next_state), ld=self.ld,
                 reward=_ptr(self.reward), index=_ptr(self.index), B=self.B, N=self.N, agent=self.agent, noise=_ptr(self.noise_t),
                 tau=C.c_float(self.tau), gamma=C.c_float(R.GAMMA), mw=self.mw, y=_ptr(self.out("y")), next_q=_ptr(self.out("next_q")),
                 next_action=_ptr(self.out("next_action")))
        a.update(ov)
        return self.lib.mdr_maddpg_target(a["actor"], a["critic"], a["next_state"], a["ld"], a["reward"], a["index"], a["B"], a["N"], a["agent"],
                                          a["noise"], a["tau"], a["gamma"], a["mw"], a["y"], a["next_q"], a["next_action"], _stream())

    def run_critic(self, y=None, **ov):
        """`y`: the device tensor the call reads (default: what run_target left)."""
        y_in = self.out("y").clone() if y is None else y
        self.ws.fill_(NAN)
        self._fill(CRITIC_OUTS)
        a = dict(critic=C.byref(self.nets["c"]), state=_ptr(self.state), ld=self.ld, action=_ptr(self.action), index=_ptr(self.index), B=self.B,
                 N=self.N, y_in=_ptr(y_in), mw=self.mw, ws=_ptr(self.ws), grad=_ptr(self.out("cgrad")), loss=_ptr(self.out("closs")),
                 q=_ptr(self.out("q")))
        a.update(ov)
        return self.lib.mdr_maddpg_critic_grad(a["critic"], a["state"], a["ld"], a["action"], a["index"], a["B"], a["N"], a["y_in"], a["mw"],
                                               a["ws"], a["grad"], a["loss"], a["q"], _stream())

    def run_actor(self, **ov):
        self.ws.fill_(NAN)
        self._fill(ACTOR_OUTS)
        a = dict(actor=C.byref(self.nets[""]), critic=C.byref(self.nets["c"]), state=_ptr(self.state), ld=self.ld, action=_ptr(self.action),
                 index=_ptr(self.index), B=self.B, N=self.N, agent=self.agent, noise=_ptr(self.noise_a), tau=C.c_float(self.tau),
                 pse=C.c_float(R.PSE), mw=self.mw, ws=_ptr(self.ws), grad=_ptr(self.out("agrad")), loss=_ptr(self.out("aloss")),
                 q=_ptr(self.out("Q")), logits=_ptr(self.out("logits")))
        a.update(ov)
        return self.lib.mdr_maddpg_actor_grad(a["actor"], a["critic"], a["state"], a["ld"], a["action"], a["index"], a["B"], a["N"], a["agent"],
                                              a["noise"], a["tau"], a["pse"], a["mw"], a["ws"], a["grad"], a["loss"], a["q"], a["logits"],
                                              _stream())

    def run(self):
        for f in (self.run_target, self.run_critic, self.run_actor):
            rc = f()
            if rc != nat.MDR_OK:
                return rc
        return nat.MDR_OK

    def results(self):
        r = {k: self.out(k).cpu().numpy() for k in ("y", "next_q", "q", "cgrad", "Q", "agrad")}
        r["next_action"] = self.out("next_action").cpu().numpy().reshape(self.B, self.N)
        r["logits"] = self.out("logits").cpu().numpy().reshape(self.B, 2)
        r["closs"], r["aloss"] = self.out("closs").cpu().numpy()[0], self.out("aloss").cpu().numpy()[0]
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
    for k in R.FLOAT_KEYS:
        w = R.worst(got[k], r["ref"][k], r["bound"][k])
        print("%s %-7s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


def _agents(N):
    return sorted({0, N // 2, N - 1})


SWEEP = [(B,) + net + (a, tau) for net in R.NETS[:4] for B in R.ROWS for a in _agents(net[0]) for tau in (1.0, 0.5)]
SWEEP += [(33,) + R.NETS[4] + (a, tau) for a in _agents(20) for tau in (1.0, 0.5)]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B%d-N%d-F%d-H%d-%d-a%d-tau%g" % c)
def test_sweep_matches_fp64_within_the_bound(case):
    r = R.reference(*case)
    call = Call(r["inputs"], case[5], case[6])
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "B%d N%d F%d H%d/%d a%d tau%g" % case)


def _case(d, agent, tau=1.0):
    return dict(inputs=d, ref=R.evaluate(d, agent, tau), bound=R.bound(d, agent, tau))


def test_two_workgroups_take_several_tiles_and_a_partial_one():
    B = 16 * 7 + 5      # 8 tiles over 2 workgroups: four each, the last one of 5 rows; the weight pass loops over its blocks as well
    r = _case(R.inputs(B, *MID), 1, 0.5)
    call = Call(r["inputs"], 1, 0.5, max_workgroups=2)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "max_workgroups=2")


def test_one_row_beyond_a_full_pass_of_the_library_grid():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * min(cus, 512) + 1
    assert B < 10 ** 5
    r = _case(R.inputs(B, *R.NETS[1]), 1)
    call = Call(r["inputs"], 1)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "B%d own grid" % B)


def test_index_equals_the_gathered_copy_bit_for_bit():
    M, B = 65, 40
    d = R.inputs(M, *MID)
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [60, 3, 60, 3]      # repeats, out of order
    rows = dict(noise_t_rows=d["noise_t"][idx], noise_a_rows=d["noise_a"][idx])
    gathered = dict(d, **{k: d[k][idx] for k in R.ROW_KEYS})
    a, b = Call(dict(d, **rows), 2, 0.5, index=_dev(idx.astype(np.int64))), Call(gathered, 2, 0.5)
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    _check(rb, _case(gathered, 2, 0.5), "gathered")


def test_strided_env_steps_and_canaries():
    B, (N, F, _, _) = 33, MID
    r = R.reference(B, *MID, 0, 1.0)
    wide = torch.full((2, B, N * F + 29), NAN, dtype=torch.float32, device=DEV)
    wide[0, :, 7:7 + N * F] = _dev(r["inputs"]["state"]).reshape(B, -1)
    wide[1, :, 7:7 + N * F] = _dev(r["inputs"]["next_state"]).reshape(B, -1)
    call = Call(r["inputs"], 0, state=wide[0, :, 7:7 + N * F], next_state=wide[1, :, 7:7 + N * F], ld=N * F + 29, pad=64)
    assert call.run() == nat.MDR_OK
    assert call.canaries_intact()
    _check(call.results(), r, "ld_state=%d" % (N * F + 29))


def test_two_calls_give_equal_bits():
    r = R.reference(65, *MID, 1, 0.5)
    call = Call(r["inputs"], 1, 0.5, max_workgroups=3)
    assert call.run() == nat.MDR_OK
    first = call.results()
    assert call.run() == nat.MDR_OK
    second = call.results()
    for k in first:
        assert np.array_equal(first[k], second[k]), k


def test_nan_in_y_reaches_the_loss_and_stays_out_of_q():
    call = Call(R.inputs(33, *MID), 1)
    assert call.run_target() == nat.MDR_OK
    y = call.out("y").clone()
    y[17] = NAN
    assert call.run_critic(y=y) == nat.MDR_OK
    got = call.results()
    s = R.param_slices(3 * 53, 100, 100, 1)
    assert np.isnan(got["closs"]) and np.isnan(got["cgrad"][s["b3"]]).all()
    assert np.isnan(got["q"]).sum() == 0


def test_zero_rows_write_zeros():
    call = Call(R.inputs(16, *MID), 1)
    assert call.run_target(B=0) == nat.MDR_OK and call.untouched(TARGET_OUTS)
    assert call.run_critic(B=0) == nat.MDR_OK
    assert bool((call.out("cgrad") == 0).all()) and float(call.out("closs")[0]) == 0.0 and call.untouched(("q",))
    assert call.run_actor(B=0) == nat.MDR_OK
    assert bool((call.out("agrad") == 0).all()) and float(call.out("aloss")[0]) == 0.0 and call.untouched(("Q", "logits"))


def _wrong(net, **fields):
    twin = nat.MdrMlp.from_buffer_copy(net)
    for k, v in fields.items():
        setattr(twin, k, v)
    return C.byref(twin)


def test_refusals_leave_every_output_untouched():
    call = Call(R.inputs(33, *MID), 1)
    N, F = call.N, call.F
    short = call.nets["c"].struct_size - 8
    for ov in (dict(actor=None), dict(critic=None), dict(next_state=None), dict(reward=None), dict(noise=None), dict(y=None), dict(next_action=None),
               dict(ld=N * F - 1), dict(B=-1), dict(mw=-1), dict(N=0), dict(N=2), dict(agent=-1), dict(agent=N), dict(tau=C.c_float(0.0)),
               dict(tau=C.c_float(NAN)), dict(gamma=C.c_float(NAN)), dict(gamma=C.c_float(float("inf"))),
               dict(actor=_wrong(call.nets["t"], struct_size=short)), dict(critic=_wrong(call.nets["tc"], w2=None))):
        assert call.run_target(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(TARGET_OUTS), ov
    for ov in (dict(actor=_wrong(call.nets["t"], hidden1=257)), dict(critic=_wrong(call.nets["tc"], hidden2=257)),
               dict(actor=_wrong(call.nets["t"], num_out=1)), dict(critic=_wrong(call.nets["tc"], num_out=2))):
        assert call.run_target(**ov) == nat.MDR_ERR_UNSUPPORTED, ov
        assert call.untouched(TARGET_OUTS), ov
    y = torch.zeros(call.B, dtype=torch.float32, device=DEV)
    for ov in (dict(critic=None), dict(state=None), dict(action=None), dict(y_in=None), dict(ws=None), dict(grad=None), dict(loss=None),
               dict(ld=N * F - 1), dict(B=-1), dict(mw=-1), dict(N=0), dict(N=2), dict(ws=C.c_void_p(call.ws.data_ptr() + 4)),
               dict(critic=_wrong(call.nets["c"], struct_size=short))):
        assert call.run_critic(y=y, **ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(CRITIC_OUTS), ov
    for ov in (dict(critic=_wrong(call.nets["c"], hidden1=257)), dict(critic=_wrong(call.nets["c"], num_out=2)),
               dict(critic=_wrong(call.nets["c"], num_state=1281), N=1, ld=1279)):
        assert call.run_critic(y=y, **ov) == nat.MDR_ERR_UNSUPPORTED, ov
        assert call.untouched(CRITIC_OUTS), ov
    for ov in (dict(actor=None), dict(critic=None), dict(state=None), dict(action=None), dict(noise=None), dict(ws=None), dict(grad=None),
               dict(loss=None), dict(ld=N * F - 1), dict(B=-1), dict(mw=-1), dict(N=2), dict(agent=-1), dict(agent=N), dict(tau=C.c_float(-1.0)),
               dict(tau=C.c_float(NAN)), dict(pse=C.c_float(NAN)), dict(ws=C.c_void_p(call.ws.data_ptr() + 8)),
               dict(actor=_wrong(call.nets[""], num_state=F - 1))):
        assert call.run_actor(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(ACTOR_OUTS), ov
    for ov in (dict(actor=_wrong(call.nets[""], hidden2=257)), dict(actor=_wrong(call.nets[""], num_out=1)),
               dict(critic=_wrong(call.nets["c"], hidden1=300))):
        assert call.run_actor(**ov) == nat.MDR_ERR_UNSUPPORTED, ov
        assert call.untouched(ACTOR_OUTS), ov
    # the optional outputs may be missing
    assert call.run_target(next_q=None) == nat.MDR_OK and call.untouched(("next_q",)) and not bool(torch.isnan(call.out("y")).any())
    assert call.run_critic(q=None) == nat.MDR_OK and call.untouched(("q",))
    assert call.run_actor(q=None, logits=None) == nat.MDR_OK and call.untouched(("Q", "logits"))
    torch.cuda.synchronize()


def _modules(d):
    from mdr_amd.maddpg import DDPGNetworkMLP
    nets = {}
    for prefix in R.PREFIXES:
        H, K = d[prefix + "W1"].shape
        net = DDPGNetworkMLP(K, d[prefix + "W3"].shape[0], H).to(DEV)
        with torch.no_grad():
            for p, k in zip((t for lin in net.fc for t in (lin.weight, lin.bias)), R.PARAM_NAMES):
                p.copy_(_dev(d[prefix + k]))
        nets[prefix] = net
    return nets


def _flat(net):
    return torch.cat([p.grad.reshape(-1) for lin in net.fc for p in (lin.weight, lin.bias)]).cpu().numpy()


def test_python_calls_fill_grad_with_what_the_c_calls_wrote():
    from mdr_amd import maddpg
    B, agent, tau = 33, 2, 0.5
    d = R.inputs(B, *MID)
    nets = _modules(d)
    call = Call(d, agent, tau)
    assert call.run() == nat.MDR_OK
    want = call.results()
    state, next_state, action, reward = (_dev(d[k]) for k in ("state", "next_state", "action", "reward"))
    y, next_q, next_action = maddpg.maddpg_target(nets["t"], nets["tc"], next_state, reward, agent, _dev(d["noise_t"]), tau, R.GAMMA)
    assert next_action.dtype == torch.uint8 and next_action.shape == (B, 3)
    for k, t in (("y", y), ("next_q", next_q), ("next_action", next_action)):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    critic, actor = nets["c"], nets[""]
    critic.fc[0].weight.grad = torch.full_like(critic.fc[0].weight, NAN)      # an existing gradient is overwritten, a missing one made
    assert critic.fc[1].weight.grad is None
    loss, q = maddpg.joint_q_loss_backward(actor, critic, state, action, y, want_q=True)
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(want["closs"])
    assert np.array_equal(q.cpu().numpy(), want["q"]) and np.array_equal(_flat(critic), want["cgrad"])
    assert all(p.grad is None for p in actor.parameters())
    before = _flat(critic).copy()
    noise = _dev(np.ascontiguousarray(d["noise_a"][:, agent, :]))
    loss, Q, logits = maddpg.actor_loss_backward(actor, critic, state, action, agent, noise, tau, R.PSE, want_q=True)
    assert float(loss) == float(want["aloss"]) and np.array_equal(Q.cpu().numpy(), want["Q"]) and np.array_equal(logits.cpu().numpy(), want["logits"])
    assert np.array_equal(_flat(actor), want["agrad"])
    assert np.array_equal(_flat(critic), before)      # the actor's call leaves the critic's .grad alone


def test_supported_and_value_errors():
    from mdr_amd import maddpg
    actor, critic = maddpg.DDPGNetworkMLP(51, 2).to(DEV), maddpg.DDPGNetworkMLP(20 * 53, 1).to(DEV)
    assert maddpg.supported(actor, critic, 20) and not maddpg.supported(actor, critic, 19)
    wide = maddpg.DDPGNetworkMLP(51, 2, 300).to(DEV)
    many = maddpg.DDPGNetworkMLP(25 * 53, 1).to(DEV)
    assert not maddpg.supported(wide, critic, 20) and not maddpg.supported(actor, many, 25) and not maddpg.supported(maddpg.DDPGNetworkMLP(51, 2), critic, 20)
    s, a, r = torch.zeros((4, 20, 51), device=DEV), torch.zeros((4, 20), dtype=torch.int64, device=DEV), torch.zeros((4, 20), device=DEV)
    with pytest.raises(ValueError, match="at most 256"):
        maddpg.maddpg_target(wide, critic, s, r, 0, torch.zeros((4, 20, 2), device=DEV))
    with pytest.raises(ValueError, match="noise"):
        maddpg.maddpg_target(actor, critic, s, r, 0, torch.zeros((4, 19, 2), device=DEV))
    with pytest.raises(ValueError, match="y must"):
        maddpg.joint_q_loss_backward(actor, critic, s, a, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="state must"):
        maddpg.actor_loss_backward(actor, critic, s[:, :, :50], a, 0, torch.zeros((4, 2), device=DEV))
