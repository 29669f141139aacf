"""mdr_amd.optim.FusedAdam on the GPU: every output element of clamp -> norm clip -> Adam -> blend within the derived bound of
tests/optim_ref.py (torch's own Adam + clip_grad_norm_, the yardstick, too), edge values, the two forms bit for bit, the state_dict
round trip with torch.optim.Adam, and every learner stepping through it."""
import numpy as np
import pytest
import torch

from mdr_amd import optim
from tests import optim_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_NORM, LR, TAU, CLAMP = 0.5, 1e-3, 0.01, 0.5
ONE, TWO = 1 << 30, 1      # max_fused_floats forcing the one-launch and the two-launch form
WORST = {}


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts]


class Net:
    """Parameters, targets and a FusedAdam over them; the gradients are slices of one flat buffer (unaligned offsets) or tensors of
    their own; `dead` names segments without a gradient."""

    def __init__(self, shapes, flat=True, dead=(), max_fused_floats=0, seed=1):
        self.shapes, self.flat, self.dead = shapes, flat, set(dead)
        self.p = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in ref.draw(shapes, seed)]
        self.target = [torch.from_numpy(x).to(DEV) for x in ref.draw(shapes, seed + 1)]
        self.opt = optim.FusedAdam(self.p, LR, max_fused_floats=max_fused_floats)
        n = sum(p.numel() for p in self.p)
        self.buf = torch.zeros(n, dtype=torch.float32, device=DEV)
        off = 0
        for i, p in enumerate(self.p):
            if i not in self.dead:
                p.grad = self.buf[off:off + p.numel()].view_as(p) if flat else torch.zeros_like(p)
            off += p.numel()

    def set_grad(self, g):
        for i, (p, x) in enumerate(zip(self.p, g)):
            if i not in self.dead:
                p.grad.copy_(torch.from_numpy(x))

    def moments(self):
        return _np(self.opt._m_views), _np(self.opt._v_views)

    def snapshot(self):
        m, v = self.moments()
        return dict(p=_np(self.p), m=m, v=v, target=_np(self.target), g=[None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in self.p])


def _check(label, before, after, norm, t, blend, clamp, clip=True):
    want, bnd = ref.bound(before["p"], before["g"], before["m"], before["v"], t, LR, target=before["target"], tau=TAU if blend else None,
                          max_norm=MAX_NORM if clip else None, clamp=CLAMP if clamp else None)
    ratios = {k: ref.worst_ratio(after[k], want[k], bnd[k]) for k in ("p", "m", "v", "target")}
    if norm is not None:
        ratios["total_norm"] = ref.worst_ratio(float(norm), want["total_norm"], bnd["total_norm"])
    for k, r in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), r)
    print("%s t=%d: worst |error| / bound %s" % (label, t, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(r <= 1.0 for r in ratios.values()), (label, t, ratios)
    return want


def _grads(shapes, t):
    return ref.draw(shapes, 100 + t, 3.0 if t % 2 == 0 else 0.001)      # 0.001 sqrt(3077) < 0.5: unclipped at every case


CASE_ARGS = [("six", True, ()), ("six", False, ()), ("ragged", True, ()), ("twenty", True, (7,)), ("ones", True, ())]


@pytest.mark.parametrize("blend", [False, True], ids=["noblend", "blend"])
@pytest.mark.parametrize("clamp", [False, True], ids=["noclamp", "clamp"])
@pytest.mark.parametrize("name,flat,dead", CASE_ARGS, ids=["six-flat", "six-own", "ragged", "twenty-one-dead", "ones"])
def test_ten_steps_each_within_the_bound(name, flat, dead, clamp, blend):
    """t = 1 from zero moments up to t = 10, gradients alternating between scale 0.001 (unclipped) and 3 (clipped): every step is
    checked against the fp64 step from the kernel's own previous fp32 state.  A dead segment stays bit for bit what it was."""
    shapes = ref.CASES[name]
    net = Net(shapes, flat=flat, dead=dead)
    if flat and name == "six":
        assert net.p[1].grad.data_ptr() % 16 != 0      # the first bias at float 35 of the flat gradient
    first = net.snapshot()
    clipped = []
    for t in range(1, 11):
        net.set_grad(_grads(shapes, t))
        before = net.snapshot()
        norm = net.opt.step(max_grad_norm=MAX_NORM, grad_clamp=CLAMP if clamp else None, target=net.target if blend else None,
                            tau=TAU if blend else None, want_norm=True)
        after = net.snapshot()
        want = _check(name, before, after, norm, t, blend, clamp)
        clipped.append(want["total_norm"] > MAX_NORM)
        for i in range(len(shapes)):      # the gradient is read, never written
            if i not in net.dead:
                assert np.array_equal(after["g"][i], before["g"][i])
        if not blend:
            assert all(np.array_equal(a, b) for a, b in zip(after["target"], first["target"]))
    assert any(clipped) and not all(clipped)
    for i in net.dead:
        for k in ("p", "m", "v", "target"):
            assert np.array_equal(after[k][i], first[k][i])
        assert net.p[i] not in net.opt.state or not net.opt.state[net.p[i]]


def test_dead_segment_with_loaded_moments_is_bit_unchanged():
    shapes = ref.CASES["twenty"]
    net = Net(shapes, dead=(7,))
    sd = net.opt.state_dict()
    m0, v0 = ref.draw(shapes, 7), [np.abs(x) for x in ref.draw(shapes, 8)]
    sd["state"] = {i: dict(step=torch.tensor(4.0), exp_avg=torch.from_numpy(m0[i]), exp_avg_sq=torch.from_numpy(v0[i])) for i in range(len(shapes))}
    net.opt.load_state_dict(sd)
    net.set_grad(_grads(shapes, 2))
    before = net.snapshot()
    assert np.array_equal(before["m"][7], m0[7]) and np.array_equal(before["v"][7], v0[7])
    norm = net.opt.step(max_grad_norm=MAX_NORM, target=net.target, tau=TAU, want_norm=True)
    after = net.snapshot()
    _check("twenty loaded", before, after, norm, 5, True, False)
    for k in ("p", "m", "v", "target"):
        assert np.array_equal(after[k][7], before[k][7])
    assert float(net.opt.state[net.p[0]]["step"]) == 5.0 and float(net.opt.state[net.p[7]]["step"]) == 4.0


@pytest.mark.parametrize("name", ["six", "ragged", "ones"])
def test_torch_adam_with_clip_grad_norm_sits_inside_the_bound(name):
    """The yardstick: a bound that torch's own fp32 step breaks would be wrong."""
    shapes = ref.CASES[name]
    for scale in (3.0, 0.01):
        p = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in ref.draw(shapes, 1)]
        target = [torch.from_numpy(x).to(DEV) for x in ref.draw(shapes, 2)]
        g = ref.draw(shapes, 5, scale)
        for q, x in zip(p, g):
            q.grad = torch.from_numpy(x).to(DEV)
        zeros = [np.zeros(s, dtype=np.float32) for s in shapes]
        before = dict(p=_np(p), g=g, m=zeros, v=zeros, target=_np(target))
        adam = torch.optim.Adam(p, LR)
        norm = torch.nn.utils.clip_grad_norm_(p, MAX_NORM)
        adam.step()
        with torch.no_grad():
            torch._foreach_mul_(target, 1.0 - TAU)
            torch._foreach_add_(target, [q.detach() for q in p], alpha=TAU)
        after = dict(p=_np(p), m=_np([adam.state[q]["exp_avg"] for q in p]), v=_np([adam.state[q]["exp_avg_sq"] for q in p]), target=_np(target))
        saved = dict(WORST)
        _check("torch " + name, before, after, norm, 1, True, False)
        WORST.clear(), WORST.update(saved)      # the yardstick's ratios are not the kernel's


def test_edge_values():
    shapes = ref.SIX
    # an all-zero gradient: p bit-unchanged, v = 0
    net = Net(shapes)
    before = net.snapshot()
    net.opt.step(max_grad_norm=MAX_NORM, target=net.target, tau=TAU)
    after = net.snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(after["p"], before["p"]))
    assert all(not a.any() for a in after["v"]) and all(not a.any() for a in after["m"])
    # a norm below max_norm: g unscaled, m of the first step = (1 - beta1) g within one rounding (of the product; the constant is a float)
    net = Net(shapes)
    g = ref.draw(shapes, 5, 0.01)
    net.set_grad(g)
    norm = net.opt.step(max_grad_norm=MAX_NORM, want_norm=True)
    assert float(norm) < MAX_NORM
    m, _ = net.moments()
    for a, x in zip(m, g):
        exact = np.float64(np.float32(1.0 - 0.9)) * x.astype(np.float64)
        assert (np.abs(a - exact) <= ref.U * np.abs(exact)).all()
    # one NaN with a clip: every live parameter NaN; without: that element alone
    for clip in (True, False):
        net = Net(shapes, dead=(3,))
        g = ref.draw(shapes, 5, 3.0)
        g[2][4, 3] = np.nan
        net.set_grad(g)
        before = net.snapshot()
        norm = net.opt.step(max_grad_norm=MAX_NORM if clip else None, want_norm=True)
        after = net.snapshot()
        assert np.isnan(float(norm))
        for i in range(len(shapes)):
            bad = np.isnan(after["p"][i])
            if i == 3:
                assert np.array_equal(after["p"][i], before["p"][i])
            elif clip:
                assert bad.all()
            else:
                want = np.zeros(shapes[i], dtype=bool)
                if i == 2:
                    want[4, 3] = True
                assert np.array_equal(bad, want)


@pytest.mark.parametrize("name", ["ragged", "six"])
def test_both_forms_and_two_calls_give_the_same_bits(name):
    shapes = ref.CASES[name]
    runs = []
    for limit in (ONE, TWO, ONE):
        net = Net(shapes, max_fused_floats=limit)
        out = []
        for t in (1, 2):
            net.set_grad(_grads(shapes, t + 1))
            norm = net.opt.step(max_grad_norm=MAX_NORM, grad_clamp=4.0, target=net.target, tau=TAU, want_norm=True)
            snap = net.snapshot()
            out.append([np.float32(float(norm))] + snap["p"] + snap["m"] + snap["v"] + snap["target"])
        runs.append(out)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def test_c_call_refusals_launch_nothing():
    import ctypes as C
    from mdr_amd import _native as nat
    lib = nat.load()
    p, g, t = (torch.ones(8, device=DEV) for _ in range(3))
    m, v = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)

    def call(table, step=1, tau=0.0, m=m):
        return lib.mdr_adam_step(C.byref(table), m.data_ptr() if m is not None else None, v.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, step, 0.5, float("inf"), tau,
                                 None, None, 0, torch.cuda.current_stream().cuda_stream)

    def table(n=1, size=None, param=p.data_ptr(), target=None):
        tb = nat.MdrAdamSegments()
        tb.struct_size = C.sizeof(nat.MdrAdamSegments) if size is None else size
        tb.nb_segments = n
        for i in range(min(n, 32)):
            tb.seg[i].param, tb.seg[i].grad, tb.seg[i].target, tb.seg[i].count = param, g.data_ptr(), target, 8 if i == 0 else 0
        return tb

    assert call(table(size=8)) == nat.MDR_ERR_INVALID
    assert call(table(n=33)) in (nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED)
    assert call(table(param=None)) == nat.MDR_ERR_INVALID
    assert call(table(), step=0) == nat.MDR_ERR_INVALID
    assert call(table(), tau=0.01) == nat.MDR_ERR_INVALID
    assert call(table(), m=None) == nat.MDR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and not bool(m.any()) and not bool(v.any())
    assert call(table(target=t.data_ptr()), tau=0.01) == nat.MDR_OK
    torch.cuda.synchronize()
    assert bool((p != 1).all()) and bool((t != 1).all()) and bool((g == 1).all())


def test_state_dict_round_trip_with_torch_adam():
    shapes = ref.SIX
    # torch -> fused
    p = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in ref.draw(shapes, 1)]
    adam = torch.optim.Adam(p, LR)
    for t in (1, 2, 3):
        for q, x in zip(p, _grads(shapes, t)):
            q.grad = torch.from_numpy(x).to(DEV)
        torch.nn.utils.clip_grad_norm_(p, MAX_NORM)
        adam.step()
    fused = optim.FusedAdam(p, LR)
    fused.load_state_dict(adam.state_dict())
    g = _grads(shapes, 4)
    for q, x in zip(p, g):
        q.grad = torch.from_numpy(x).to(DEV)
    before = dict(p=_np(p), g=g, m=_np([adam.state[q]["exp_avg"] for q in p]), v=_np([adam.state[q]["exp_avg_sq"] for q in p]), target=None)
    norm = fused.step(max_grad_norm=MAX_NORM, want_norm=True)
    after = dict(p=_np(p), m=_np([fused.state[q]["exp_avg"] for q in p]), v=_np([fused.state[q]["exp_avg_sq"] for q in p]))
    want, bnd = ref.bound(before["p"], g, before["m"], before["v"], 4, LR, max_norm=MAX_NORM)
    for k in ("p", "m", "v"):
        assert ref.worst_ratio(after[k], want[k], bnd[k]) <= 1.0, k
    assert ref.worst_ratio(float(norm), want["total_norm"], bnd["total_norm"]) <= 1.0
    assert all(float(fused.state[q]["step"]) == 4.0 for q in p)
    # fused -> torch
    back = torch.optim.Adam(p, LR)
    back.load_state_dict(fused.state_dict())
    g = _grads(shapes, 5)
    for q, x in zip(p, g):
        q.grad = torch.from_numpy(x).to(DEV)
    before = dict(p=_np(p), m=after["m"], v=after["v"])
    norm = torch.nn.utils.clip_grad_norm_(p, MAX_NORM)
    back.step()
    got = dict(p=_np(p), m=_np([back.state[q]["exp_avg"] for q in p]), v=_np([back.state[q]["exp_avg_sq"] for q in p]))
    want, bnd = ref.bound(before["p"], g, before["m"], before["v"], 5, LR, max_norm=MAX_NORM)
    for k in ("p", "m", "v"):
        assert ref.worst_ratio(got[k], want[k], bnd[k]) <= 1.0, k
    assert all(float(back.state[q]["step"]) == 5.0 for q in p)


# ---- the learners ---------------------------------------------------------------------------------------------------------------------
class Spy:
    """Wraps FusedAdam.step on one optimiser: records (p, g, m, v, target, t) before and the result after every call, and checks each
    call against the fp64 step of that one call."""

    def __init__(self, opt, label):
        self.opt, self.label, self.calls = opt, label, 0
        self.inner = opt.step
        opt.step = self

    def __call__(self, max_grad_norm=None, grad_clamp=None, target=None, tau=None, want_norm=False):
        opt = self.opt
        params = opt._params
        live = [p.grad is not None for p in params]
        st = opt.state.get(params[live.index(True)])
        t = int(st["step"]) + 1 if st else 1
        before = dict(p=_np(params), g=_np([p.grad for p in params]), m=_np(opt._m_views), v=_np(opt._v_views), target=_np(target) if target is not None else None)
        norm = self.inner(max_grad_norm=max_grad_norm, grad_clamp=grad_clamp, target=target, tau=tau, want_norm=True)
        after = dict(p=_np(params), m=_np(opt._m_views), v=_np(opt._v_views), target=_np(target) if target is not None else None)
        want, bnd = ref.bound(before["p"], before["g"], before["m"], before["v"], t, opt.param_groups[0]["lr"], target=before["target"], tau=tau,
                              max_norm=max_grad_norm, clamp=grad_clamp)
        keys = ("p", "m", "v") + (("target",) if target is not None else ())
        ratios = {k: ref.worst_ratio(after[k], want[k], bnd[k]) for k in keys}
        ratios["total_norm"] = ref.worst_ratio(float(norm), want["total_norm"], bnd["total_norm"])
        for k, r in ratios.items():
            WORST[k] = max(WORST.get(k, 0.0), r)
        assert all(r <= 1.0 for r in ratios.values()), (self.label, self.calls, ratios)
        assert all(np.array_equal(a, b) for a, b, l in zip(_np([p.grad for p in params]), before["g"], live) if l)
        self.calls += 1
        return norm if want_norm else None


def _no_torch_tail(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("clip_grad_norm_ on the FusedAdam path")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", boom)


def _tiny_env(N=3, E=2):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=11)
    env.reset(episode=0)
    return env


@pytest.mark.parametrize("kind", ["ppo", "mappo"])
def test_ppo_and_mappo_learners_step_through_fused_adam(kind, monkeypatch):
    from mdr_amd import mappo, ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP, collect_ppo_rollout
    env = _tiny_env()
    F = env.obs_vector_length()
    torch.manual_seed(1)
    actor = ActorMLP(F, layers=(12, 10)).to(DEV)
    critic = CriticMLP(F + (2 if kind == "mappo" else 0), layers=(12, 10)).to(DEV)
    if kind == "mappo":
        batch = collect_ppo_rollout(env, actor, 2, with_others_actions=True, seed=3)
        learner = mappo.MAPPOLearner(actor, critic, 1e-3, 3e-3, batch_size=4, ppo_update_time=2, backend="hip", optimizer=optim.FusedAdam)
    else:
        batch = collect_ppo_rollout(env, actor, 2, critic=critic, seed=3)
        learner = ppo.PPOLearner(actor, critic, 1e-3, 3e-3, batch_size=4, ppo_update_time=2, backend="hip", optimizer=optim.FusedAdam)
    assert isinstance(learner.actor_optimizer, optim.FusedAdam) and isinstance(learner.critic_optimizer, optim.FusedAdam)
    spies = [Spy(learner.actor_optimizer, kind + " actor"), Spy(learner.critic_optimizer, kind + " critic")]
    seen = []
    learner.before_clip = lambda lrn: seen.append(1)
    _no_torch_tail(monkeypatch)
    a_loss, c_loss, count = learner.update(batch, seed=0)
    assert count == 2 * 3 and len(seen) == count and all(s.calls == count for s in spies)      # 12 transitions in minibatches of 4
    assert bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
    assert actor.fc[0].bias.grad.data_ptr() == actor._mdr_flat_grad.data_ptr() + 4 * actor.fc[0].weight.numel()


def test_one_fused_and_one_torch_optimiser_mix(monkeypatch):
    from mdr_amd import ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP, collect_ppo_rollout
    env = _tiny_env()
    F = env.obs_vector_length()
    torch.manual_seed(1)
    actor, critic = ActorMLP(F, layers=(12, 10)).to(DEV), CriticMLP(F, layers=(12, 10)).to(DEV)
    batch = collect_ppo_rollout(env, actor, 2, critic=critic, seed=3)
    learner = ppo.PPOLearner(actor, critic, 1e-3, 3e-3, batch_size=4, ppo_update_time=1, backend="hip")
    learner.actor_optimizer = optim.FusedAdam(actor.parameters(), 1e-3)
    spy = Spy(learner.actor_optimizer, "mixed actor")
    clips = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda params, *a, **k: (clips.append(list(params)), real(clips[-1], *a, **k))[1])
    learner.update(batch, seed=0)
    assert spy.calls == 3 and len(clips) == 3
    assert all(all(any(q is c for c in critic.parameters()) for q in ps) for ps in clips)      # the critic alone went through torch's clip


def test_tarmac_learner_steps_through_fused_adam(monkeypatch):
    from mdr_amd import tarmac_ppo as tp
    from mdr_amd.rollout import collect_tarmac_rollout
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    N, E, T = 3, 2, 2
    env = _tiny_env(N, E)
    F = env.obs_vector_length()
    torch.manual_seed(11)
    actor, critic = TarMACActor(F).to(DEV), TarMACCritic(N, F).to(DEV)
    ro = collect_tarmac_rollout(env, actor, T, gamma=0.9, critic=critic, seed=5)
    learner = tp.TarMACPPOLearner(actor, critic, lr_actor=1e-3, lr_critic=1e-3, backend="hip", optimizer=optim.FusedAdam, ppo_update_time=2,
                                  batch_size=4, max_grad_norm=0.5)
    spies = [Spy(learner.actor_optimizer, "tarmac actor"), Spy(learner.critic_optimizer, "tarmac critic")]
    _no_torch_tail(monkeypatch)
    untouched = [p.detach().clone() for p in actor.comm.msg_state2state.parameters()]
    a_loss, c_loss, count = learner.update(ro, seed=1)
    assert count == 2 and all(s.calls == count for s in spies)      # T E = 4 env-steps: one minibatch per epoch
    assert bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
    assert all(p.grad is None and torch.equal(p, q) for p, q in zip(actor.comm.msg_state2state.parameters(), untouched))
    assert len(learner.actor_optimizer.state_dict()["state"]) == 20      # the one-hop actor's 20 live tensors of 24


def _dqn(double, **kw):
    from mdr_amd.dqn import DQNLearner, QNetworkMLP
    from mdr_amd.rollout import collect_dqn_transitions
    env = _tiny_env()
    torch.manual_seed(1)
    net = QNetworkMLP(env.obs_vector_length(), 2, (12, 10)).to(DEV)
    batch = collect_dqn_transitions(env, net, 2, epsilon=0.5, seed=3)
    twin = QNetworkMLP(env.obs_vector_length(), 2, (12, 10)).to(DEV)
    twin.load_state_dict(net.state_dict())
    learner = DQNLearner(twin, 1e-3, buffer_capacity=64, batch_size=4, double=double, backend="hip", optimizer=optim.FusedAdam, **kw)
    learner.store(batch)
    return learner


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
def test_dqn_learner_steps_and_blends_through_fused_adam(double, monkeypatch):
    learner = _dqn(double, tau=0.01)
    spy = Spy(learner.optimizer, "ddqn" if double else "dqn")
    seen = []
    learner.before_step = lambda lrn: seen.append(1)
    _no_torch_tail(monkeypatch)

    def boom(*a, **k):
        raise AssertionError("a separate blend on the FusedAdam path")
    monkeypatch.setattr(learner, "update_target_network", boom)
    monkeypatch.setattr(torch, "_foreach_mul_", boom)
    old = [p.detach().clone() for p in learner.target_net.parameters()]
    for _ in range(3):
        assert bool(torch.isfinite(learner.update(seed=0)))
    assert spy.calls == 3 and len(seen) == 3 and learner.training_step == 3
    assert all(not torch.equal(a, b) for a, b in zip(learner.target_net.parameters(), old))      # blended, inside the one launch
    still = _dqn(double, tau=0.01, soft_update=False)
    old = [p.detach().clone() for p in still.target_net.parameters()]
    still.update(seed=0)
    assert all(torch.equal(a, b) for a, b in zip(still.target_net.parameters(), old))


def test_twenty_fused_updates_against_a_fixed_target_lower_the_td_loss():
    from mdr_amd.dqn import QNetworkMLP
    learner = _dqn(False, tau=0.0)
    buf = learner.buffer

    def td_loss():
        p64, t64 = (QNetworkMLP(buf.num_state, 2, (12, 10)).to(DEV).double() for _ in range(2))
        p64.load_state_dict(learner.policy_net.state_dict()), t64.load_state_dict(frozen)
        n = len(buf)
        with torch.no_grad():
            y = buf.reward[:n].double().view(-1, 1) + t64(buf.next_state[:n].double()).max(1)[0].unsqueeze(1) * learner.gamma
            return float(torch.nn.SmoothL1Loss()(p64(buf.state[:n].double()).gather(1, buf.action[:n].view(-1, 1)), y))

    frozen = {k: v.clone() for k, v in learner.target_net.state_dict().items()}
    learner.batch_size = len(buf)
    before = td_loss()
    losses = [learner.update(seed=0) for _ in range(20)]
    after = td_loss()
    print("FusedAdam: fp64 Huber TD loss over the buffer %.6f -> %.6f" % (before, after))
    assert all(bool(torch.isfinite(l)) for l in losses) and learner.training_step == 20
    assert all(torch.equal(v, frozen[k]) for k, v in learner.target_net.state_dict().items())      # tau = 0: no blend
    assert after < before


def test_zz_report_worst_ratios():
    """Last in the file: the worst |error| / bound the kernel reached over every check above (profiles/optim_step_README.md quotes it)."""
    print("worst |error| / bound over this file: " + "  ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert max(WORST.values(), default=0.0) <= 1.0
