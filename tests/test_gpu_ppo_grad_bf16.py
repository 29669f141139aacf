"""mdr_ppo_actor_grad_bf16x3 / mdr_ppo_critic_grad_bf16x3 (include/mdr_policy.h, csrc/mdr_ppo_grad_bf16.hip) and
mdr_amd.ppo(precision="bf16x3") on the GPU, against the exact fp64 values and the derived bound of tests/ppo_grad_bf16_ref.py: every
element of every output, worst |error| / bound <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import ppo_grad_bf16_ref as br
from tests import ppo_grad_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
HEADS = pytest.mark.parametrize("O", [2, 1], ids=["actor", "critic"])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Call:
    """One call of the C entry point on device copies of a case's inputs; every output and the workspace NaN-filled first.  `index`
    (numpy int64): the rows of the buffers the minibatch takes; the actor's advantage is `adv`, in minibatch order."""

    def __init__(self, d, O, max_workgroups=0, index=None, adv=None):
        self.lib = nat.load()
        self.O, self.mw = O, max_workgroups
        self.suffix = "_bf16x3"      # "": the fp32 entry point with the same argument list
        self.params = [_dev(d[k]) for k in pr.PARAM_NAMES]
        H1, F = d["W1"].shape
        self.net = nat.MdrMlp(C.sizeof(nat.MdrMlp), F, H1, d["W2"].shape[0], O, *[_ptr(p) for p in self.params])
        self.state, self.ld = _dev(d["x"]), F
        self.index = _dev(np.asarray(index, dtype=np.int64)) if index is not None else None
        self.B = int(len(index)) if index is not None else int(d["x"].shape[0])
        self.whole = [_dev(d[k]) for k in (("action", "old") if O == 2 else ("target",))]
        self.adv_in = _dev(d["adv"] if adv is None else adv) if O == 2 else None
        self.G = int(self.lib.mdr_mlp_grad_floats(C.byref(self.net)))
        nbytes = int(self.lib.mdr_mlp_grad_workspace_bytes(C.byref(self.net), self.B, max_workgroups))
        assert self.G > 0 and nbytes > 0
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        self.bufs = {k: torch.empty(n, dtype=torch.float32, device=DEV) for k, n in (("grad", self.G), ("loss", 1), ("out0", self.B), ("out1", self.B))}

    def run(self, **override):
        self.ws.fill_(NAN)
        for b in self.bufs.values():
            b.fill_(NAN)
        a = dict(net=C.byref(self.net), state=_ptr(self.state), ld=self.ld, index=_ptr(self.index), B=self.B, w0=_ptr(self.whole[0]),
                 w1=_ptr(self.whole[1]) if self.O == 2 else None, adv=_ptr(self.adv_in), clip=C.c_float(pr.CLIP), mw=self.mw,
                 ws=_ptr(self.ws), grad=_ptr(self.bufs["grad"]), loss=_ptr(self.bufs["loss"]), out0=_ptr(self.bufs["out0"]),
                 out1=_ptr(self.bufs["out1"]))
        a.update(override)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.O == 2:
            return getattr(self.lib, "mdr_ppo_actor_grad" + self.suffix)(a["net"], a["state"], a["ld"], a["index"], a["B"], a["w0"], a["w1"], a["adv"], a["clip"],
                                                      a["mw"], a["ws"], a["grad"], a["loss"], a["out0"], stream)
        return getattr(self.lib, "mdr_ppo_critic_grad" + self.suffix)(a["net"], a["state"], a["ld"], a["index"], a["B"], a["w0"], a["mw"], a["ws"], a["grad"],
                                                   a["loss"], a["out0"], a["out1"], stream)

    def results(self):
        r = dict(grad=self.bufs["grad"].cpu().numpy(), loss=self.bufs["loss"].cpu().numpy()[0])
        if self.O == 2:
            r["ratio"] = self.bufs["out0"].cpu().numpy()
        else:
            r["value"], r["advantage"] = self.bufs["out0"].cpu().numpy(), self.bufs["out1"].cpu().numpy()
        return r

    def untouched(self):
        return bool(torch.isnan(self.ws).all()) and all(bool(torch.isnan(b).all()) for b in self.bufs.values())


def _check(got, ref, bnd, label, keys=None):
    for k in (keys or bnd):
        w = pr.worst(got[k], ref[k], bnd[k])
        print("%s %-9s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


@HEADS
@pytest.mark.parametrize("case", br.SWEEP, ids=lambda c: "B%d-F%d-H%d-%d" % c)
def test_sweep_matches_fp64_within_the_bound(case, O):
    r = br.reference(*case, O)
    call = Call(r["inputs"], O)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r["ref"], r["bound"], "B%d F%d H%d/%d O%d" % (case + (O,)))


@HEADS
@pytest.mark.parametrize("kind,case", br.SWEEP_KINDS, ids=lambda v: v if isinstance(v, str) else "B%d-F%d-H%d-%d" % v)
def test_sweep_of_the_further_grid_kinds(kind, case, O):
    """Tails in x ("x") and in W2 ("w2"): the cross terms the first grid leaves at zero - x's tail in F1 and dW1, W2's in F2 and B2."""
    r = br.reference(*case, O, kind)
    call = Call(r["inputs"], O)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r["ref"], r["bound"], "%s B%d F%d H%d/%d O%d" % ((kind,) + case + (O,)))


@HEADS
@pytest.mark.parametrize("net", [(51, 100, 100), (8, 16, 16), (63, 97, 113)], ids=lambda n: "F%d-H%d-%d" % n)
def test_partials_lie_where_the_fp32_entry_point_puts_them(net, O):
    """mdr_mlp_grad_workspace_bytes sizes the workspace of both precisions from the fp32 file's grid and stride: both entry points
    must write the same floats of it - as many partials, as far apart, each as long - and none behind it."""
    for B, mw in ((33, 0), (257, 0), (257, 1), (257, 3), (100, 64)):
        call = Call(br.inputs(B, *net, O), O, max_workgroups=mw)
        n = call.ws.numel()
        call.ws = torch.empty(2 * n + 64, dtype=torch.float32, device=DEV)      # the sized part, then canaries
        written = {}
        for name, call.suffix in (("bf16x3", "_bf16x3"), ("fp32", "")):
            assert call.run() == nat.MDR_OK
            written[name] = ~torch.isnan(call.ws)
            assert not bool(written[name][n:].any()), (name, B, mw)
        assert bool(written["bf16x3"].any()) and torch.equal(written["bf16x3"], written["fp32"]), (B, mw)


@HEADS
@pytest.mark.parametrize("mw", [1, 2, 0])
def test_every_grid_is_within_the_bound_and_repeats_its_bits(mw, O):
    r = br.reference(257, 51, 100, 100, O)      # on one workgroup: all 17 tiles, the last of one row
    call = Call(r["inputs"], O, max_workgroups=mw)
    assert call.run() == nat.MDR_OK
    first = call.results()
    _check(first, r["ref"], r["bound"], "max_workgroups=%d O%d" % (mw, O))
    assert call.run() == nat.MDR_OK
    second = call.results()
    for k in first:
        assert np.array_equal(first[k], second[k]), k


@HEADS
def test_index_equals_the_gathered_copy_bit_for_bit(O):
    M, B = 257, 100
    d = br.inputs(M, 51, 100, 100, O)
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [200, 3, 200, 3]      # repeats, out of order
    gathered = br.take_rows(d, idx)
    if O == 2:
        gathered["adv"] = d["adv"][:B]      # the advantage is in minibatch order in both calls
    a = Call(d, O, index=idx, adv=d["adv"][:B] if O == 2 else None)
    b = Call(gathered, O)
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    _check(rb, pr.evaluate(gathered), br.bound(gathered), "gathered O%d" % O)


@HEADS
@pytest.mark.parametrize("net", [(51, 100, 100), (64, 128, 128), (63, 97, 113)], ids=lambda n: "F%d-H%d-%d" % n)
def test_full_mantissa_inputs(net, O):
    r = br.full_reference(*net, O)
    label = "full F%d H%d/%d O%d" % (net + (O,))
    # forward outputs over all 257 rows: within the forward bound of the exact fp64 values
    call = Call(r["inputs"], O)
    assert call.run() == nat.MDR_OK
    got = call.results()
    _check(got, r["fwd_exact"], r["fwd_bound"], label + " all rows", br.FORWARD_KEYS[O])
    # the gradient on the rows whose ReLU masks are not a matter of rounding, taken through `index`
    keep, kept = r["keep"], r["kept"]
    print("%s: %d of %d rows left out" % (label, br.PARENT_ROWS - len(keep), br.PARENT_ROWS))
    assert 3 * (br.PARENT_ROWS - len(keep)) <= br.PARENT_ROWS
    call = Call(r["inputs"], O, index=keep, adv=kept["inputs"]["adv"] if O == 2 else None)
    assert call.run() == nat.MDR_OK
    _check(call.results(), kept["ref"], kept["bound"], label + " kept rows")


@HEADS
def test_refusals_leave_everything_untouched(O):
    d = br.inputs(33, 51, 100, 100, O)
    call = Call(d, O)
    invalid = [dict(net=None), dict(state=None), dict(grad=None), dict(loss=None), dict(ws=None), dict(w0=None), dict(ld=50), dict(B=-1),
               dict(mw=-1), dict(ws=C.c_void_p(call.ws.data_ptr() + 4))]
    if O == 2:
        invalid += [dict(w1=None), dict(adv=None), dict(clip=C.c_float(-0.1)), dict(clip=C.c_float(1.0)), dict(clip=C.c_float(NAN))]
    for ov in invalid:
        assert call.run(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(), ov
    for field, value in (("num_state", 65), ("hidden1", 129), ("hidden2", 129), ("num_out", 3 - O), ("num_out", 3)):
        net = nat.MdrMlp.from_buffer_copy(call.net)
        setattr(net, field, value)
        assert call.run(net=C.byref(net), ld=128) == nat.MDR_ERR_UNSUPPORTED, (field, value)
        assert call.untouched(), (field, value)
    torch.cuda.synchronize()


def test_zero_rows_write_zeros():
    call = Call(br.inputs(16, 51, 100, 100, 2), 2)
    assert call.run(B=0) == nat.MDR_OK
    assert bool((call.bufs["grad"] == 0).all()) and float(call.bufs["loss"][0]) == 0.0


def _modules(F=51, layers=(100, 100), seed=0):
    from mdr_amd.rollout import ActorMLP, CriticMLP
    torch.manual_seed(seed)
    return ActorMLP(F, layers=layers).to(DEV), CriticMLP(F, layers=layers).to(DEV)


def test_python_calls_fill_grad_with_what_the_c_call_wrote():
    from mdr_amd import ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP
    B, F, H1, H2 = 65, 51, 100, 100
    for O in (2, 1):
        d = br.inputs(B, F, H1, H2, O)
        net = (ActorMLP(F, layers=(H1, H2)) if O == 2 else CriticMLP(F, layers=(H1, H2))).to(DEV)
        with torch.no_grad():
            for lin, (w, b) in zip(net.fc, (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
                lin.weight.copy_(_dev(d[w]))
                lin.bias.copy_(_dev(d[b]))
        call = Call(d, O)
        assert call.run() == nat.MDR_OK
        want = call.results()
        if O == 2:
            loss, ratio = ppo.actor_loss_backward(net, _dev(d["x"]), _dev(d["action"]), _dev(d["old"]), _dev(d["adv"]), pr.CLIP, want_ratio=True,
                                                  precision="bf16x3")
            assert np.array_equal(ratio.cpu().numpy(), want["ratio"])
        else:
            loss, value, adv = ppo.critic_loss_backward(net, _dev(d["x"]), _dev(d["target"]), precision="bf16x3")
            assert np.array_equal(value.cpu().numpy(), want["value"]) and np.array_equal(adv.cpu().numpy(), want["advantage"])
        assert float(loss) == float(want["loss"])
        got = torch.cat([p.grad.reshape(-1) for lin in net.fc for p in (lin.weight, lin.bias)]).cpu().numpy()
        assert np.array_equal(got, want["grad"])


def test_python_value_errors():
    from mdr_amd import ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP
    actor, critic = _modules()
    assert ppo.supported(actor, precision="bf16x3") and ppo.supported(critic, precision="bf16x3")
    assert ppo.refusal(actor, 2, precision="bf16x3") is None
    big = ActorMLP(64, layers=(128, 128)).to(DEV)
    assert ppo.supported(big, precision="bf16x3")      # no shape inside the limits is refused
    wide = ActorMLP(81, layers=(100, 100)).to(DEV)
    fat = CriticMLP(51, layers=(100, 200)).to(DEV)
    assert not ppo.supported(wide, precision="bf16x3") and not ppo.supported(fat, precision="bf16x3")
    x = torch.zeros((4, 51), device=DEV)
    a, p, adv = torch.zeros(4, dtype=torch.int64, device=DEV), torch.ones(4, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(ValueError, match="'fp32' or 'bf16x3'"):
        ppo.actor_loss_backward(actor, x, a, p, adv, precision="bf16")
    with pytest.raises(ValueError, match="'fp32' or 'bf16x3'"):
        ppo.supported(actor, precision="fp16")
    with pytest.raises(ValueError, match="wide=True"):
        ppo.critic_loss_backward(critic, x, p, wide=True, precision="bf16x3")
    with pytest.raises(ValueError, match="at most 64 input features"):
        ppo.actor_loss_backward(wide, torch.zeros((4, 81), device=DEV), a, p, adv, precision="bf16x3")
    with pytest.raises(ValueError, match="at most 128"):
        ppo.critic_loss_backward(fat, x, p, precision="bf16x3")
    # the learner: a refused network, backend="torch", wide=True, an unknown value
    with pytest.raises(ValueError, match="at most 64 input features"):
        ppo.PPOLearner(wide, critic, 1e-3, 1e-3, precision="bf16x3")
    with pytest.raises(ValueError, match="at most 128"):
        ppo.PPOLearner(actor, fat, 1e-3, 1e-3, backend="auto", precision="bf16x3")
    with pytest.raises(ValueError, match="backend='torch'"):
        ppo.PPOLearner(actor, critic, 1e-3, 1e-3, backend="torch", precision="bf16x3")
    with pytest.raises(ValueError, match="wide=True"):
        ppo.PPOLearner(actor, critic, 1e-3, 1e-3, wide=True, precision="bf16x3")
    with pytest.raises(ValueError, match="'fp32' or 'bf16x3'"):
        ppo.PPOLearner(actor, critic, 1e-3, 1e-3, precision="tf32")
    cfg = dict(lr_actor=1e-3, lr_critic=1e-3, clip_param=0.2, max_grad_norm=0.5, ppo_update_time=2, batch_size=64)
    assert ppo.PPOLearner.from_config(cfg, actor, critic, precision="bf16x3").precision == "bf16x3"
    assert ppo.PPOLearner.from_config(cfg, actor, critic).precision == "fp32"
    assert ppo.PPOLearner(actor, critic, 1e-3, 1e-3, backend="auto").precision == "fp32"      # "auto" never picks bf16x3 by itself


def _clone(net):
    """A fresh module with the same parameters (collect_ppo_rollout leaves its packed kernel operands on the actor: no deepcopy)."""
    from mdr_amd.rollout import ActorMLP
    F = net.fc[0].in_features
    twin = type(net)(F, 2, net.layers) if isinstance(net, ActorMLP) else type(net)(F, net.layers)
    twin.load_state_dict(net.state_dict())
    return twin.to(DEV)


def _fp64_losses(actor, critic, batch, clip):
    """agents/ppo.py:148-169, 180 over the whole batch in fp64."""
    T = batch["state"].shape[0] - 1
    state = batch["state"][:T].reshape(-1, batch["state"].shape[-1])
    action, old, target = batch["action"].reshape(-1), batch["a_prob"].reshape(-1), batch["return"].reshape(-1)
    a64, c64 = _clone(actor).double(), _clone(critic).double()
    with torch.no_grad():
        s = state.double()
        V = c64(s)
        Gt = target.double().view(-1, 1)
        adv = Gt - V
        ratio = a64(s).gather(1, action.view(-1, 1)) / old.double().view(-1, 1)
        a_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
        return float(a_loss), float(torch.nn.functional.mse_loss(Gt, V))


@pytest.fixture(scope="module")
def rollout():
    import mdr_amd
    from mdr_amd.rollout import collect_ppo_rollout
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=4, device=DEV, seed=11)
    env.reset(episode=0)
    actor, critic = _modules(env.obs_vector_length(), seed=1)
    batch = collect_ppo_rollout(env, actor, 8, critic=critic, seed=3)
    return actor, critic, batch


def _learner(rollout, **kw):
    from mdr_amd import ppo
    actor0, critic0, _ = rollout
    return ppo.PPOLearner(_clone(actor0), _clone(critic0), 1e-3, 3e-3, batch_size=256, ppo_update_time=2, **kw)


def _params(learner):
    return [p.detach().clone() for net in (learner.actor, learner.critic) for p in net.parameters()]


def test_learner_lowers_both_losses_as_the_fp32_learner_does(rollout):
    batch = rollout[2]
    after = {}
    for precision in ("fp32", "bf16x3"):
        learner = _learner(rollout, backend="hip", precision=precision)
        before = _fp64_losses(learner.actor, learner.critic, batch, learner.clip_param)
        a_loss, c_loss, count = learner.update(batch, seed=0)
        assert count == 6 and a_loss.is_cuda and a_loss.dim() == 0
        after[precision] = _fp64_losses(learner.actor, learner.critic, batch, learner.clip_param)
        print("%s: actor loss %.6f -> %.6f, critic loss %.6f -> %.6f" % (precision, before[0], after[precision][0], before[1], after[precision][1]))
        assert after[precision][0] < before[0] and after[precision][1] < before[1]
        assert all(bool(torch.isfinite(p).all()) for p in _params(learner))
    # the same descent: what the two precisions gained differs by far less than the gain
    for i in (0, 1):
        gain = before[i] - after["fp32"][i]
        assert abs(after["bf16x3"][i] - after["fp32"][i]) < 0.01 * gain


def test_graph_replays_the_eager_philox_bits_with_one_capture(rollout):
    from mdr_amd.optim import FusedAdam
    batch = rollout[2]
    eager = _learner(rollout, backend="hip", precision="bf16x3", sampler="philox", optimizer=FusedAdam)
    graph = _learner(rollout, backend="hip", precision="bf16x3", graph=True, optimizer=FusedAdam)
    fp32 = _learner(rollout, backend="hip", sampler="philox", optimizer=FusedAdam)
    for seed in (0, 1):
        e, g = eager.update(batch, seed=seed), graph.update(batch, seed=seed)
        fp32.update(batch, seed=seed)
        assert e[2] == g[2] and torch.equal(e[0], g[0]) and torch.equal(e[1], g[1])
    assert graph.graph_captures == 1
    assert all(torch.equal(p, q) for p, q in zip(_params(eager), _params(graph)))
    assert not all(torch.equal(p, q) for p, q in zip(_params(eager), _params(fp32)))      # the graph replays the bf16x3 launches


def test_precision_fp32_is_the_learner_without_the_argument(rollout):
    batch = rollout[2]
    plain, named = _learner(rollout, backend="hip"), _learner(rollout, backend="hip", precision="fp32")
    p, n = plain.update(batch, seed=0), named.update(batch, seed=0)
    assert torch.equal(p[0], n[0]) and torch.equal(p[1], n[1])
    assert all(torch.equal(a, b) for a, b in zip(_params(plain), _params(named)))
