"""mdr_mappo_critic_grad (include/mdr_policy.h) and mdr_amd.mappo on the GPU, against the fp64 restatement and the derived rounding
bound of tests/mappo_grad_ref.py / tests/ppo_grad_ref.py: every element of every output, worst |error| / bound <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import mappo_grad_ref as mr
from tests import ppo_grad_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
REF = (51, 20, 100, 100)      # the reference's shape: 51 features, 20 agents, hidden 100-100


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Call:
    """One call of the C entry point on device copies of a case's buffer; every output and the workspace NaN-filled first."""

    def __init__(self, d, N, B=None, max_workgroups=0, index=None, state=None, ld=None, pad=0):
        self.lib = nat.load()
        self.N, self.mw = N, max_workgroups
        self.params = [_dev(d[k]) for k in pr.PARAM_NAMES]
        H1, J = d["W1"].shape
        H2 = d["W2"].shape[0]
        self.F = J - (N - 1)
        self.net = nat.MdrMlp(C.sizeof(nat.MdrMlp), J, H1, H2, 1, *[_ptr(p) for p in self.params])
        self.state = _dev(d["state"]) if state is None else state
        self.ld = self.F if ld is None else ld
        self.action, self.target = _dev(d["action"]), _dev(d["buffer_target"])
        self.M = int(d["action"].shape[0])
        self.index = index
        self.B = int(index.shape[0]) if index is not None else (int(d["x"].shape[0]) if B is None else B)
        self.G = int(self.lib.mdr_mappo_critic_grad_floats(C.byref(self.net), N))
        self.pad = pad      # canary floats on either side of every output
        nbytes = int(self.lib.mdr_mappo_critic_workspace_bytes(C.byref(self.net), N, self.B, max_workgroups))
        assert self.G == H1 * J + H1 + H2 * H1 + H2 + H2 + 1 and nbytes > 0
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        self.bufs = {k: torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV)
                     for k, n in (("grad", self.G), ("loss", 1), ("value", self.B), ("advantage", self.B))}

    def out(self, k):
        b = self.bufs[k]
        return b[self.pad:b.numel() - self.pad]

    def run(self, **override):
        self.ws.fill_(NAN)
        for b in self.bufs.values():
            b.fill_(NAN)
        a = dict(net=C.byref(self.net), state=_ptr(self.state), ld=self.ld, action=_ptr(self.action), M=self.M, N=self.N, index=_ptr(self.index),
                 B=self.B, target=_ptr(self.target), mw=self.mw, ws=_ptr(self.ws), grad=_ptr(self.out("grad")), loss=_ptr(self.out("loss")),
                 value=_ptr(self.out("value")), advantage=_ptr(self.out("advantage")))
        a.update(override)
        return self.lib.mdr_mappo_critic_grad(a["net"], a["state"], a["ld"], a["action"], a["M"], a["N"], a["index"], a["B"], a["target"], a["mw"],
                                              a["ws"], a["grad"], a["loss"], a["value"], a["advantage"],
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def results(self):
        return dict(grad=self.out("grad").cpu().numpy(), loss=self.out("loss").cpu().numpy()[0], value=self.out("value").cpu().numpy(),
                    advantage=self.out("advantage").cpu().numpy())

    def untouched(self):
        return all(bool(torch.isnan(b).all()) for b in self.bufs.values())

    def canaries_intact(self):
        p = self.pad
        return all(bool(torch.isnan(b[:p]).all()) and bool(torch.isnan(b[b.numel() - p:]).all()) for b in self.bufs.values())


def _check(got, r, label):
    for k in r["bound"]:
        w = pr.worst(got[k], r["ref"][k], r["bound"][k])
        print("%s %-9s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


@pytest.mark.parametrize("case", mr.SWEEP, ids=lambda c: "B%d-F%d-N%d-H%d-%d" % c)
def test_sweep_matches_fp64_within_the_bound(case):
    r = mr.reference(*case)
    call = Call(r["inputs"], case[2])
    assert call.M >= call.B and call.M % case[2] == 0
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "B%d F%d N%d H%d/%d" % case)


def test_two_workgroups_take_several_tiles_and_a_partial_one():
    B = 16 * 7 + 5      # 8 tiles over 2 workgroups: four each, the last one of 5 rows
    r = mr.reference(B, *REF)
    call = Call(r["inputs"], REF[1], max_workgroups=2)
    assert call.run() == nat.MDR_OK
    _check(call.results(), r, "max_workgroups=2")


def test_index_equals_the_gathered_copy_bit_for_bit():
    F, N, H1, H2 = REF
    M, B = 13 * N, 100
    full = mr.case(M, F, N, H1, H2, M=M)["inputs"]      # x: the joint rows of the whole buffer
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:8] = [M - 1, 0, N - 1, M - N, M - 1, 0, 200, 3]      # agent 0 and agent N - 1 of the first and the last env; repeats, out of order
    # the gathered copy: minibatch row i's whole env group at rows i N .. i N + N - 1, the row itself at its agent's place
    group = (idx - idx % N)[:, None] + np.arange(N)[None, :]
    gathered = dict(full, state=full["state"][group.reshape(-1)], action=full["action"][group.reshape(-1)],
                    buffer_target=full["buffer_target"][group.reshape(-1)])
    a = Call(full, N, index=_dev(idx.astype(np.int64)))
    b = Call(gathered, N, index=_dev((np.arange(B) * N + idx % N).astype(np.int64)))
    assert a.run() == nat.MDR_OK and b.run() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    d = dict(full, x=full["x"][idx], target=full["buffer_target"][idx])
    _check(ra, dict(ref=pr.evaluate(d), bound=pr.bound(d)), "index")


def test_strided_states_and_canaries():
    B = 65
    r = mr.reference(B, *REF)
    F, M = REF[0], r["inputs"]["state"].shape[0]
    wide = torch.full((M, 80), NAN, dtype=torch.float32, device=DEV)
    wide[:, 7:7 + F] = _dev(r["inputs"]["state"])
    call = Call(r["inputs"], REF[1], state=wide[:, 7:7 + F], ld=80, pad=64)
    assert call.run() == nat.MDR_OK
    assert call.canaries_intact()
    _check(call.results(), r, "ld_state=80")


def test_two_calls_give_equal_bits():
    r = mr.reference(257, *REF)
    call = Call(r["inputs"], REF[1], max_workgroups=3)
    assert call.run() == nat.MDR_OK
    first = call.results()
    assert call.run() == nat.MDR_OK
    second = call.results()
    for k in first:
        assert np.array_equal(first[k], second[k]), k


def test_zero_rows_write_zeros():
    call = Call(mr.reference(16, *REF)["inputs"], REF[1])
    assert call.run(B=0) == nat.MDR_OK
    assert bool((call.out("grad") == 0).all()) and float(call.out("loss")[0]) == 0.0


def test_refusals_leave_the_outputs_untouched():
    F, N = REF[:2]
    call = Call(mr.reference(33, *REF)["inputs"], N)
    invalid = [dict(net=None), dict(state=None), dict(action=None), dict(target=None), dict(grad=None), dict(loss=None), dict(ws=None),
               dict(N=0), dict(N=-1), dict(N=F + N), dict(ld=F - 1), dict(M=call.M + 1), dict(M=call.M - 1), dict(B=-1), dict(mw=-1),
               dict(ws=C.c_void_p(call.ws.data_ptr() + 4))]
    for ov in invalid:
        assert call.run(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(), ov
    size = nat.MdrMlp.from_buffer_copy(call.net)
    size.struct_size -= 8
    assert call.run(net=C.byref(size)) == nat.MDR_ERR_INVALID and call.untouched()
    # the shape alone is refused: nb_agents keeps F = 51 where the width changes, M = 0 is a multiple of every nb_agents
    for fields, agents in ((dict(num_out=2), N), (dict(num_state=129), 79), (dict(hidden1=129), N), (dict(hidden2=129), N),
                           (dict(num_state=101), 51), (dict(num_state=69, hidden1=128, hidden2=128), 19)):
        net = nat.MdrMlp.from_buffer_copy(call.net)
        for field, value in fields.items():
            setattr(net, field, value)
        assert call.run(net=C.byref(net), N=agents, M=0) == nat.MDR_ERR_UNSUPPORTED, fields
        assert call.untouched(), fields
    assert call.run(value=None, advantage=None) == nat.MDR_OK      # the two optional outputs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(call.out("grad")).all()) and bool(torch.isnan(call.out("value")).all())


def _critic_with(d, F, N, H1, H2):
    from mdr_amd.rollout import CriticMLP
    net = CriticMLP(F + N - 1, layers=(H1, H2)).to(DEV)
    with torch.no_grad():
        for lin, (w, b) in zip(net.fc, (("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            lin.weight.copy_(_dev(d[w]))
            lin.bias.copy_(_dev(d[b]))
    return net


def test_python_call_fills_grad_with_what_the_c_call_wrote():
    from mdr_amd import mappo
    B = 65
    F, N, H1, H2 = REF
    d = mr.reference(B, *REF)["inputs"]
    M = d["action"].shape[0]
    idx = _dev(np.arange(B, dtype=np.int64))
    call = Call(d, N, index=idx)
    assert call.run() == nat.MDR_OK
    want = call.results()
    net = _critic_with(d, *REF)
    net.fc[0].weight.grad = torch.full_like(net.fc[0].weight, NAN)      # an existing gradient is overwritten, a missing one made
    loss, value, adv = mappo.joint_critic_loss_backward(net, _dev(d["state"]), _dev(d["action"]), _dev(d["buffer_target"]), index=idx)
    assert np.array_equal(value.cpu().numpy(), want["value"]) and np.array_equal(adv.cpu().numpy(), want["advantage"])
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(want["loss"])
    got = torch.cat([p.grad.reshape(-1) for lin in net.fc for p in (lin.weight, lin.bias)]).cpu().numpy()
    assert np.array_equal(got, want["grad"])
    assert M % N == 0


def test_supported_and_value_errors():
    from mdr_amd import mappo, ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP
    critic = CriticMLP(70).to(DEV)
    assert mappo.supported(critic, 51) and not ppo.supported(critic)
    assert mappo.supported(CriticMLP(100).to(DEV), 51) and mappo.supported(CriticMLP(128, layers=(64, 64)).to(DEV), 64)
    assert not mappo.supported(CriticMLP(101).to(DEV), 51)                 # the LDS layout
    assert not mappo.supported(CriticMLP(129, layers=(64, 64)).to(DEV), 64)
    assert not mappo.supported(critic, 71) and not mappo.supported(CriticMLP(70), 51)
    state = torch.zeros((40, 51), device=DEV)
    action, target = torch.zeros(40, dtype=torch.int64, device=DEV), torch.zeros(40, device=DEV)
    with pytest.raises(ValueError, match="LDS"):
        mappo.joint_critic_loss_backward(CriticMLP(101).to(DEV), state, action, target)
    with pytest.raises(ValueError, match="at most 128 input features"):
        mappo.joint_critic_loss_backward(CriticMLP(180).to(DEV), state, action, target)
    with pytest.raises(ValueError, match="no whole number of env-steps"):
        mappo.joint_critic_loss_backward(critic, state[:39], action[:39], target[:39])
    with pytest.raises(ValueError, match="agents"):
        mappo.joint_critic_loss_backward(critic, state, action, target, nb_agents=10)
    with pytest.raises(ValueError, match="backend='hip'"):
        mappo.MAPPOLearner(ActorMLP(51).to(DEV), CriticMLP(101).to(DEV), 1e-3, 1e-3, backend="hip")
    loss, value, adv = mappo.joint_critic_loss_backward(critic, state, action, target)
    assert value.shape == (40,) and bool(torch.isfinite(loss))


def _clone(net):
    """A fresh module with the same parameters (collect_ppo_rollout leaves its packed kernel operands on the actor: no deepcopy)."""
    from mdr_amd.rollout import ActorMLP
    F = net.fc[0].in_features
    twin = type(net)(F, 2, net.layers) if isinstance(net, ActorMLP) else type(net)(F, net.layers)
    twin.load_state_dict(net.state_dict())
    return twin.to(DEV)


def _fp64_losses(actor, critic, state, action, old, target, others, clip):
    """agents/mappo.py:85-104, 113 over the whole batch in fp64."""
    a64, c64 = _clone(actor).double(), _clone(critic).double()
    with torch.no_grad():
        s = state.double()
        V = c64(torch.cat((s, others.double()), 1))
        Gt = target.double().view(-1, 1)
        adv = Gt - V
        ratio = a64(s).gather(1, action.view(-1, 1)) / old.double().view(-1, 1)
        a_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
        return float(a_loss), float(torch.nn.functional.mse_loss(Gt, V))


@pytest.fixture(scope="module")
def rollout():
    import mdr_amd
    from mdr_amd.rollout import ActorMLP, CriticMLP, collect_ppo_rollout
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=4, device=DEV, seed=11)
    env.reset(episode=0)
    F = env.obs_vector_length()
    torch.manual_seed(1)
    actor, critic = ActorMLP(F, layers=(100, 100)).to(DEV), CriticMLP(F + 19, layers=(100, 100)).to(DEV)
    batch = collect_ppo_rollout(env, actor, 8, with_others_actions=True, seed=3)
    return actor, critic, batch


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_learner_end_to_end(rollout, backend):
    from mdr_amd import mappo, ppo
    actor0, critic0, batch = rollout
    bare = {k: v for k, v in batch.items() if k != "others_actions"}
    prop = dict(lr_actor=1e-3, lr_critic=3e-3, clip_param=0.2, max_grad_norm=0.5, ppo_update_time=2, batch_size=256)
    actor, critic = _clone(actor0), _clone(critic0)
    learner = mappo.MAPPOLearner.from_config(prop, actor, critic, backend=backend)
    assert learner.nb_agents == 20 and learner.uses_kernels(256) == (backend == "hip")
    T = batch["state"].shape[0] - 1
    state = batch["state"][:T].reshape(-1, batch["state"].shape[-1])
    action, old, target = batch["action"].reshape(-1), batch["a_prob"].reshape(-1), batch["return"].reshape(-1)
    others = batch["others_actions"].reshape(-1, 19)
    n = state.shape[0]
    assert n == 8 * 80
    # (a) the same minibatch indices for the same seed, whatever the backend
    other = mappo.MAPPOLearner.from_config(prop, _clone(actor0), _clone(critic0), backend="torch" if backend == "hip" else "hip")
    for epoch in range(2):
        mine, theirs = learner.minibatches(n, 0, epoch), other.minibatches(n, 0, epoch)
        assert [len(b) for b in mine] == [256, 256, 128] and all(torch.equal(p, q) for p, q in zip(mine, theirs))
    before = _fp64_losses(actor, critic, state, action, old, target, others, learner.clip_param)
    if backend == "hip":
        # (b) the gradients of the first minibatch, before the clipping, are those of the direct calls, bit for bit
        seen = {}

        def hook(lrn):
            if not seen:
                seen["actor"] = [p.grad.clone() for p in lrn.actor.parameters()]
                seen["critic"] = [p.grad.clone() for p in lrn.critic.parameters()]
        a2, c2 = _clone(actor0), _clone(critic0)
        idx = learner.minibatches(n, 0, 0)[0]
        _, _, adv = mappo.joint_critic_loss_backward(c2, state, action, target, index=idx)
        ppo.actor_loss_backward(a2, state, action, old, adv, learner.clip_param, index=idx)
        learner.before_clip = hook
    a_loss, c_loss, count = learner.update(batch, seed=0)
    assert count == 6 and a_loss.is_cuda and c_loss.is_cuda and a_loss.dim() == 0
    if backend == "hip":
        for got, net in ((seen["actor"], a2), (seen["critic"], c2)):
            for g, p in zip(got, net.parameters()):
                assert torch.equal(g, p.grad)
    # (c) the batch without the others_actions key gives the same parameters, bit for bit
    twin = mappo.MAPPOLearner.from_config(prop, _clone(actor0), _clone(critic0), backend=backend)
    a_bare, c_bare, _ = twin.update(bare, seed=0)
    assert torch.equal(a_bare, a_loss) and torch.equal(c_bare, c_loss)
    for mine, theirs in ((actor, twin.actor), (critic, twin.critic)):
        assert all(torch.equal(p, q) for p, q in zip(mine.parameters(), theirs.parameters()))
    # (d) both losses over the whole batch, in fp64 at the original a_prob and returns, are lower than before
    after = _fp64_losses(actor, critic, state, action, old, target, others, learner.clip_param)
    print("%s: actor loss %.6f -> %.6f, critic loss %.6f -> %.6f" % ((backend, before[0], after[0], before[1], after[1])))
    assert after[0] < before[0] and after[1] < before[1]
    assert all(bool(torch.isfinite(p).all()) for net in (actor, critic) for p in net.parameters())
    with pytest.raises(ValueError, match="whole number of envs"):
        learner.update({k: v[:, :79] for k, v in bare.items()}, seed=0)
