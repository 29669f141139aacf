"""Loader and yardstick of the learner fixtures tests/golden/learner_*.npz (oracle/learner_golden.py recorded them by running the
REFERENCE's own ``update()``, once in float32 - ``ref32`` - and once as an fp64 twin - ``ref64``).  Shared by
tests/test_learner_golden.py (CPU) and tests/test_gpu_learner_golden.py.

Loader.  A fixture is mapped to this project's layouts: the reference indexes PPO's flat buffer agent-major (a T + t), the project
step-major (t A + a), so the recorded minibatch index lists and ``Gt`` are remapped; MAPPO's buffer is step-major in both;
MADDPG's recorded noise is stored in the [N, B, N + 1, 2] layout of ``MADDPGLearner.draws`` per update (the target picks in agent
order, then the actor's own draw).  The recorded draws replace a learner's own sampler by overriding, on the instance, the method
it already calls (``minibatches`` / ``sample`` / ``draws``).

Yardstick for parameters and per-step scalars.  Per net, d_ref32 = max over its tensors and the recorded checkpoints of
|ref32 - ref64|: the reference's own float32 noise.  A run passes if its distance to ref64, taken the same way, is at most
FACTOR x d_ref32; the same per scalar series (each loss, each gradient norm).  The run under test evaluates the same expressions in
float32 in another summation order: noise of the same law and scale, where a wrong term (a divisor, a clip side, a bias correction, a
blend too many) moves a parameter by about lr per step, 1e-3 against 1e-7.

Bound for the first-minibatch gradients: the derived per-element bounds of tests/ppo_grad_ref.py, tests/dqn_grad_ref.py and
tests/maddpg_grad_ref.py / maddpg_agents_ref.py (``_maddpg_critic``; the actors: ``maddpg_actor_grad_ratios``) on the fixture's inputs, the truth being the reference's fp64 gradient.  Those bounds take a kernel's inputs as exact; against the
reference's fp64 run three inputs are not, and each adds its first-order term (``_sensitivity``: the gradient is linear in the
per-row output gradient dl, so an error E_r on a row's factor adds at most sum_r E_r |d grad / d factor_r|):
  * the critic regresses on the float32 ``Gt`` where the reference's fp64 run has its own: E_t = |Gt32 - Gt64| on the target;
  * the actor's advantage comes from the critic kernel: E_A = the critic bound's ``advantage`` + E_t;
  * the DQN kernels take gamma as a float: |0.99 - float32(0.99)| |next_q| on the TD target.
TarMAC-PPO: the critic as above with tests/tarmac_critic_ref.py; the actor by tests/tarmac_ppo_ref.py's own contract (per tensor,
relative L2 error at most max(8 x the float32 reference's, 2^-20)), with the reference's recorded float32 and fp64 gradients.
"""
import contextlib
import functools

import numpy as np

from oracle import learner_golden as rec
from tests import dqn_grad_ref as dq
from tests import maddpg_agents_ref as ma
from tests import maddpg_grad_ref as mg
from tests import ppo_grad_ref as pr

FACTOR = 4.0
CASES = rec.CASES
FC_KEYS = rec.FC_KEYS


class Fixture:
    """One case's arrays; ``f64(key)`` rejoins a float64 array stored in two parts."""

    def __init__(self, case, arrays=None):
        self.case = case
        if arrays is None:
            with np.load(rec.path(case), allow_pickle=False) as z:
                arrays = {k: z[k] for k in z.files}
        self.a = arrays
        self.kind = str(np.asarray(arrays["meta/kind"]).item())

    def __getitem__(self, key):
        return self.a[key]

    def meta(self, key):
        return self.a["meta/" + key].item()

    def f64(self, key):
        return rec.join64(self.a[key], self.a[key + "@lo"])

    def nets(self):
        return sorted({k.split("/")[2] for k in self.a if k.startswith("ref64/last/")})

    def keys(self, net):
        if self.kind == "tarmac":      # the reference modules' own state_dict keys, in their order
            net = net[4:] if net.startswith("tgt_") else net
            return [k.split("/", 2)[2] for k in self.a if k.startswith("init/%s/" % net)]
        return rec.NET_KEYS if self.kind == "maddpg" else FC_KEYS

    def init(self, net):
        """The initial state_dict; a target net starts as a copy of its source."""
        net = net[4:] if net.startswith("tgt_") else net
        return {k: self.a["init/%s/%s" % (net, k)] for k in self.keys(net)}

    def grid(self, net, prefix=""):
        return {prefix + g: v for g, v in zip(rec.GRID_KEYS, self.init(net).values())}

    def checkpoint(self, tag, ck, net):
        """{key: float64 array of the kept positions}."""
        if tag == "ref32":
            return {k: self.a["ref32/%s/%s/%s" % (ck, net, k)].astype(np.float64) for k in self.keys(net)}
        return {k: self.f64("ref64/%s/%s/%s" % (ck, net, k)) for k in self.keys(net)}

    def series(self, tag):
        """{name: float64 [steps]}: each loss and each gradient norm."""
        loss = self.f64(tag + "/loss")
        out = {"loss/" + str(n): loss[:, i] for i, n in enumerate(self.a["meta/loss_names"])}
        for k in self.a:
            if k.startswith(tag + "/norm/") and not k.endswith("@lo"):
                out["norm/" + k.split("/")[2]] = self.f64(k)
        return out


@functools.lru_cache(maxsize=None)
def fixture(case):
    return Fixture(case)


# -- the project's layouts ------------------------------------------------------------------------------------------------------------
def ppo_layout(fx):
    """-> dict(state [T + 1, A, F], action, a_prob, reward, done [T, A], Gt32, Gt64 [T, A], index: per epoch the minibatches' int64
    arrays in the project's flat order t A + a) - numpy."""
    T, A = fx.meta("T"), fx.meta("A")
    index = [row[row >= 0] for row in fx["draws/index"]]
    if fx.kind == "ppo":      # the reference's r = a T + t
        index = [(r % T) * A + r // T for r in index]
        order = lambda g: g.reshape(A, T).T.copy()
    else:
        order = lambda g: g.reshape(T, A).copy()
    epochs, i = [], 0
    for n in fx["draws/per_epoch"]:
        epochs.append(index[i:i + int(n)])
        i += int(n)
    return dict(state=fx["in/state"], action=fx["in/action"], a_prob=fx["in/a_prob"], reward=fx["in/reward"], done=fx["in/done"],
                Gt32=order(fx.f64("ref32/Gt")).astype(np.float32), Gt64=order(fx.f64("ref64/Gt")), index=epochs)


def mappo_others(action, N):
    """train_mappo.py:79-84 on [T, N] actions -> [T N, N - 1]."""
    T = action.shape[0]
    return np.array([[action[t, k] for k in range(N) if k != a] for t in range(T) for a in range(N)], dtype=np.float32)


def first_minibatch(fx):
    """The inputs of the grad_ref modules at the first minibatch, from the fixture alone.  PPO / MAPPO: (critic dict, actor dict
    without 'adv'); DQN: the one dict of dqn_grad_ref."""
    if fx.kind in ("ppo", "mappo"):
        lay = ppo_layout(fx)
        T, A, F = fx.meta("T"), fx.meta("A"), fx.meta("F")
        idx = lay["index"][0][0]
        x = lay["state"][:T].reshape(T * A, F)
        xc = x if fx.kind == "ppo" else np.concatenate([x, mappo_others(lay["action"], fx.meta("nb_agents"))], axis=1)
        critic = dict(fx.grid("critic"), x=xc[idx], target=lay["Gt64"].reshape(-1)[idx], target32=lay["Gt32"].reshape(-1)[idx])
        actor = dict(fx.grid("actor"), x=x[idx], action=lay["action"].reshape(-1)[idx], old=lay["a_prob"].reshape(-1)[idx])
        return critic, actor
    idx = fx["draws/index"][0]
    d = dict(fx.grid("policy"), **fx.grid("policy", "t"))
    d.update(x=fx["in/state"][idx], xn=fx["in/next_state"][idx], action=fx["in/action"][idx], reward=fx["in/reward"][idx], clamp=1.0)
    return d


@contextlib.contextmanager
def exact_gamma(gamma):
    """dqn_grad_ref / maddpg_grad_ref with the reference's gamma (a Python float) instead of the float the kernels' ABI takes."""
    saved = dq.GAMMA, mg.GAMMA
    dq.GAMMA = mg.GAMMA = float(gamma)
    try:
        yield
    finally:
        dq.GAMMA, mg.GAMMA = saved


def own(fx, agent):
    """The index of the nets agent ``agent`` uses (shared: the one set)."""
    return 0 if fx.meta("shared") else agent


def maddpg_first(fx, agent):
    """maddpg_grad_ref's dict for agent ``agent``'s minibatch of the first update, every net at its initial weights (the targets are
    copies), and every agent's target actor for maddpg_agents_ref."""
    N = fx.meta("nb_agents")
    idx, noise = fx["draws/index"][0, agent], fx["draws/noise"][0, agent]
    k = own(fx, agent)
    d = dict(state=fx["in/state"][idx], next_state=fx["in/next_state"][idx], action=fx["in/action"][idx], reward=fx["in/reward"][idx],
             noise_t=noise[:, :N], noise_a=np.repeat(noise[:, N:N + 1], N, axis=1))
    for prefix, net in (("", "actor%d" % k), ("t", "actor%d" % k), ("c", "critic%d" % k), ("tc", "critic%d" % k)):
        d.update(fx.grid(net, prefix))
    return d, [fx.grid("actor%d" % own(fx, j)) for j in range(N)]


def _maddpg_critic(fx, agent):
    """Agent ``agent``'s critic step of the first update where its critic is still at its initial weights: the reference's fp64
    loss and gradient, the restatement's (maddpg_agents_ref's per-agent target, then maddpg_grad_ref's critic lines) and the bound
    (maddpg_grad_ref.bound's critic part around that target; the float gamma adds |0.99 - float32(0.99)| |next_q| to E_y)."""
    d, nets = maddpg_first(fx, agent)
    tau, gamma = fx.meta("gumbel_tau"), fx.meta("gamma")
    B = d["state"].shape[0]
    with exact_gamma(gamma):
        tgt = ma.evaluate(d, nets, agent, tau)
    E_y = ma.bound(d, nets, agent, tau)["y"] + np.abs(tgt["next_q"]) * abs(gamma - mg.GAMMA)
    xc = mg.joint(np.asarray(d["state"], dtype=np.float64), d["action"])
    fwc = pr.forward(mg._net(d, "c", xc), np.float64)
    cW2, cW3 = (np.asarray(d["c" + k], dtype=np.float64) for k in ("W2", "W3"))
    q = fwc["l"][:, 0]
    delta = q - tgt["y"]
    dl = (2 * delta / B)[:, None]
    grad, _ = mg._backward(dl, fwc, xc, cW2, cW3, np.float64, False, None)
    E_delta = mg.logit_bound(d, "c", xc)[:, 0] + E_y + mg.U * np.abs(delta)
    E_dl = (2 * E_delta / B)[:, None] + 3 * mg.U * np.abs(dl)
    E_term = 2 * np.abs(delta) * E_delta + mg.U * delta * delta
    name = "critic%d" % own(fx, agent)
    names = [str(n) for n in fx["meta/loss_names"]]
    out = dict(loss=fx.f64("ref64/loss")[0][names.index("critic%d" % agent)], grad=fx.f64("ref64/grad/" + name), restated_loss=(delta * delta).mean(),
               restated_grad=grad, loss_bound=(E_term.sum() + (B + 2) * mg.U * (delta * delta).sum()) / B,
               grad_bound=mg._grad_bound(dl, E_dl, fwc, xc, cW2, cW3)[0], loss_column=names.index("critic%d" % agent))
    if fx.meta("shared"):      # the shared case is maddpg_grad_ref.evaluate's own
        with exact_gamma(gamma):
            e = mg.evaluate(d, agent, tau)
        out.update(module_loss=e["closs"], module_grad=e["cgrad"])
    return name, out


def tarmac_first(fx):
    """tarmac_critic_ref's dict (the whole buffer, target = the twin's Gt) and the first minibatch's env-steps."""
    lay = ppo_layout(fx)
    T = fx.meta("T")
    d = dict({g: fx["init/critic/critic.%d.%s" % (2 * i, w)] for i in range(3) for w, g in (("weight", "W%d" % (i + 1)), ("bias", "b%d" % (i + 1)))},
             state=lay["state"][:T], target=lay["Gt64"], target32=lay["Gt32"])
    return d, lay["index"][0][0], lay


def tarmac_actor(fx, dtype):
    """The project's TarMACActor (CPU, dense attention) on the fixture's initial weights."""
    import torch
    from mdr_amd.tarmac import TarMACActor
    actor = TarMACActor(fx.meta("F"), num_key=fx.meta("K"), num_value=fx.meta("V"), hidden_state_size=fx.meta("H"), number_agents_comm=fx.meta("c"),
                        comm_mode="neighbours", comm_defect_prob=0.0, num_hops=1, with_comm=True, attention="dense")
    actor.load_state_dict({k: torch.from_numpy(np.array(fx["init/actor/" + k])) for k in fx.keys("actor")}, strict=True)
    return actor.to(dtype)


def _named(fx, flat):
    """A flat actor gradient (the reference's parameter order, without the unreached comm.msg_state2state) -> {name: array}."""
    out, off = {}, 0
    for n in fx["meta/actor_grad_names"]:
        shape = fx["init/actor/" + str(n)].shape
        size = int(np.prod(shape))
        out[str(n)] = np.asarray(flat[off:off + size], dtype=np.float64).reshape(shape)
        off += size
    assert off == len(flat)
    return out


def _tarmac_reference(fx):
    """The critic as the other learners' (tarmac_critic_ref's derived bound, plus the float32 Gt's term); the actor by
    tarmac_ppo_ref's contract: per tensor, relative L2 error at most max(8 x that of the reference's own float32 gradient, 2^-20)
    (``holds``), the loss likewise - under tarmac_ppo_ref's ReLU condition, which ``conditions`` asserts."""
    import torch
    from tests import tarmac_critic_ref as tc
    from tests import tarmac_ppo_ref as tp
    d, idx, lay = tarmac_first(fx)
    B, N = len(idx), fx.meta("nb_agents")
    loss64, loss32 = fx.f64("ref64/loss")[0], fx.f64("ref32/loss")[0]
    ec, bc = tc.evaluate(d, np.float64, index=idx), tc.bound(d, index=idx)
    E_t = np.abs(d["target32"].astype(np.float64) - d["target"])[idx]
    net = dict({k: d[k] for k in rec.GRID_KEYS}, x=np.asarray(d["state"], dtype=np.float64)[idx].reshape(B, -1))
    extra = 0.0
    for o in range(N):      # dV[:, o] = -2 delta[:, o] / (B N): the target's error on one agent's column at a time
        unit = np.zeros((B, N))
        unit[:, o] = -2.0 / N
        extra = extra + _sensitivity(net, unit, E_t[:, o])
    out = {"critic": dict(loss=loss64[1], grad=fx.f64("ref64/grad/critic"), restated_loss=ec["loss"], restated_grad=ec["grad"],
                          loss_bound=bc["loss"] + (2 * np.abs(ec["advantage"]) * E_t).sum() / (B * N), grad_bound=bc["grad"] + extra)}
    a64 = tarmac_actor(fx, torch.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    T = fx.meta("T")
    rl, ratio, rg = tp._evaluate(a64, t(lay["state"][:T][idx]), t(lay["action"][idx]), t(lay["a_prob"][idx]), t(ec["advantage"]), None)
    g64, g32 = _named(fx, fx.f64("ref64/grad/actor")), _named(fx, fx["ref32/grad/actor"])
    out["actor"] = dict(loss=loss64[0], grad=fx.f64("ref64/grad/actor"), restated_loss=rl,
                        restated_grad=np.concatenate([rg[str(n)].reshape(-1) for n in fx["meta/actor_grad_names"]]),
                        named=dict(grad=g64, yard=tp.rel_l2(g32, g64)), loss_yard=abs(loss32[0] - loss64[0]), ratio=ratio, adv=ec["advantage"])
    return out


def _sensitivity(net, dl_unit, E):
    """sum_r E_r |d grad / d factor_r| / B for a per-row output gradient dl_r = factor_r dl_unit_r (flat, torch's parameter order)."""
    fw = pr.forward(net, np.float64)
    x, W2, W3 = (np.asarray(net[k], dtype=np.float64) for k in ("x", "W2", "W3"))
    B = x.shape[0]
    dz2 = (dl_unit @ W3) * (fw["z2"] > 0)
    dz1 = (dz2 @ W2) * (fw["z1"] > 0)
    one = np.ones((B, 1))
    w = np.asarray(E, dtype=np.float64)[:, None]
    parts = [(np.abs(dz) * w).T @ np.abs(inp) / B for dz, inp in ((dz1, x), (dz1, one), (dz2, fw["h1"]), (dz2, one), (dl_unit, fw["h2"]), (dl_unit, one))]
    return np.concatenate([p.reshape(-1) for p in parts])


@functools.lru_cache(maxsize=None)
def first_minibatch_reference(case):
    """-> {net: dict(loss, grad, loss_bound, grad_bound, restated_loss, restated_grad)}: the reference's fp64 loss and gradient of
    the first minibatch, the derived bound around them (module docstring) and the grad_ref module's own fp64 evaluation."""
    fx = fixture(case)
    loss64 = fx.f64("ref64/loss")[0]
    out = {}
    if fx.kind == "tarmac":
        return _tarmac_reference(fx)
    if fx.kind == "maddpg":
        for agent in range(1 if fx.meta("shared") else fx.meta("nb_agents")):
            name, r = _maddpg_critic(fx, agent)
            out[name] = r
        return out
    if fx.kind in ("ppo", "mappo"):
        critic, actor = first_minibatch(fx)
        B = critic["x"].shape[0]
        ec = pr.evaluate(critic, np.float64)
        bc = pr.bound(critic)
        E_t = np.abs(critic["target32"].astype(np.float64) - critic["target"])
        adv = ec["advantage"]
        out["critic"] = dict(loss=loss64[1], grad=fx.f64("ref64/grad/critic"), restated_loss=ec["loss"], restated_grad=ec["grad"],
                             loss_bound=bc["loss"] + (2 * np.abs(adv) * E_t).sum() / B,
                             grad_bound=bc["grad"] + _sensitivity(critic, np.full((B, 1), -2.0), E_t))
        actor = dict(actor, adv=adv)
        ea = pr.evaluate(actor, np.float64)
        ba = pr.bound(actor)
        E_A = bc["advantage"] + E_t
        clip = fx.meta("clip_param")
        ratio = ea["ratio"]
        s1, s2 = ratio * adv, np.clip(ratio, 1 - clip, 1 + clip) * adv
        active = ((ratio >= 1 - clip) & (ratio <= 1 + clip)) | (s1 < s2)
        rows, a = np.arange(B), actor["action"]
        fw = pr.forward(actor, np.float64)
        p_b = 1 / (1 + np.exp(fw["l"][rows, a] - fw["l"][rows, 1 - a]))
        unit = np.zeros((B, 2))
        unit[rows, a] = np.where(active, -ratio * p_b, 0)
        unit[rows, 1 - a] = -unit[rows, a]
        out["actor"] = dict(loss=loss64[0], grad=fx.f64("ref64/grad/actor"), restated_loss=ea["loss"], restated_grad=ea["grad"],
                            loss_bound=ba["loss"] + (np.maximum(np.abs(ratio), np.abs(np.clip(ratio, 1 - clip, 1 + clip))) * E_A).sum() / B,
                            grad_bound=ba["grad"] + _sensitivity(actor, unit, E_A), E_A=E_A, adv=adv, ratio=ratio)
    else:
        d = first_minibatch(fx)
        double = fx.kind == "ddqn"
        B = d["x"].shape[0]
        with exact_gamma(fx.meta("gamma")):
            e = dq.evaluate(d, np.float64, double=double)
        b = dq.bound(d, double)
        E_g = np.abs(e["next_q"]) * abs(fx.meta("gamma") - dq.GAMMA)
        unit = np.zeros((B, 2))
        unit[np.arange(B), d["action"]] = 1.0
        net = dict({g: d[g] for g in rec.GRID_KEYS}, x=d["x"])
        out["policy"] = dict(loss=loss64[0], grad=fx.f64("ref64/grad/policy"), restated_loss=e["loss"], restated_grad=e["grad"],
                             loss_bound=b["loss"] + E_g.sum() / B, grad_bound=b["grad"] + _sensitivity(net, unit, E_g), q=e["q"], y=e["y"])
    return out


# -- what the data must exercise ------------------------------------------------------------------------------------------------------
def conditions(fx):
    """Asserts the conditions the issue's table sets for the case, and the preconditions of the derived bounds."""
    if fx.kind == "tarmac":
        import torch
        from tests import tarmac_ppo_ref as tp
        lay = ppo_layout(fx)
        old, T = lay["a_prob"], fx.meta("T")
        assert (old > 0.02).all() and (old <= 0.98).all()
        assert [len(i) for i in lay["index"][0]] == [5, 5, 2] and len(lay["index"]) == 2
        ref = _tarmac_reference(fx)
        ratio, adv, clip = ref["actor"]["ratio"], ref["actor"]["adv"], fx.meta("clip_param")
        clipped = ((ratio < 1 - clip) & (adv < 0)) | ((ratio > 1 + clip) & (adv > 0))
        assert 0.1 <= clipped.mean() <= 0.6, "clip share %.2f" % clipped.mean()
        assert (np.abs(ratio - (1 - clip)) >= 1e-3).all() and (np.abs(ratio - (1 + clip)) >= 1e-3).all()
        margin = tp._relu_margin(tarmac_actor(fx, torch.float64), torch.from_numpy(lay["state"][:T]).double(), None)
        assert margin > tp.RELU_MARGIN, "tarmac_ppo_ref's ReLU condition: %.2e" % margin
        last = lay["done"].astype(bool)
        assert last[-1].all() and not last[:-1].any() and (np.abs(fx["ref32/bootstrap"][-1]) > 1e-3).all(), "the bootstrap value must be nonzero"
        return
    if fx.kind in ("ppo", "mappo"):
        lay = ppo_layout(fx)
        old = lay["a_prob"]
        assert (old > 0.02).all() and (old <= 0.98).all()
        critic, actor = first_minibatch(fx)
        adv = pr.evaluate(critic, np.float64)["advantage"]
        ratio = pr.evaluate(dict(actor, adv=adv), np.float64)["ratio"]
        clip = fx.meta("clip_param")
        clipped = ((ratio < 1 - clip) & (adv < 0)) | ((ratio > 1 + clip) & (adv > 0))
        assert 0.1 <= clipped.mean() <= 0.6, "clip share %.2f" % clipped.mean()
        assert (np.abs(ratio - (1 - clip)) >= 1e-3).all() and (np.abs(ratio - (1 + clip)) >= 1e-3).all()
        E_A = pr.bound(critic)["advantage"] + np.abs(critic["target32"].astype(np.float64) - critic["target"])
        assert (np.abs(adv) > 2 * E_A).all(), "an advantage's sign is a matter of rounding"
        last = lay["done"].astype(bool)
        boot = lay["Gt64"][last] - lay["reward"][last].astype(np.float64)
        if fx.kind == "ppo" and not fx.meta("zero_eoepisode_return"):
            assert last[-1].all() and not last[:-1].any() and (np.abs(boot) > 1e-3).all(), "the bootstrap value must be nonzero"
        else:
            assert np.abs(boot).max() < 1e-6
        if fx.kind == "mappo":
            others = mappo_others(lay["action"], fx.meta("nb_agents"))
            assert ((others == 0).any(axis=0) & (others == 1).any(axis=0)).all()
        sizes = [len(i) for i in lay["index"][0]]
        assert sizes == ([50, 50, 20] if fx.kind == "ppo" else [16, 16, 8]) and len(lay["index"]) == 2
        return
    if fx.kind == "maddpg":
        N, tau = fx.meta("nb_agents"), fx.meta("gumbel_tau")
        assert fx["draws/index"].shape == (3, N, 24) and not fx["in/action"].all(axis=0).any() and fx["in/action"].any(axis=0).all()
        for a in range(N):
            d, nets = maddpg_first(fx, a)
            assert not ma.pick_bad(d, nets, tau).any(), "a target pick is a matter of rounding"
            t, E = mg.t_bound(d, "", d["state"][:, a], d["noise_a"][:, a], tau)
            assert (np.abs(t[:, 0] - t[:, 1]) > 2 * (E[:, 0] + E[:, 1])).all(), "an actor's pick is a matter of rounding"
            pick = t[:, 1] > t[:, 0]      # before critic a's step, which the actor's logits do not depend on
            assert pick.any() and not pick.all(), "agent %d's straight-through sample holds one action only" % a
        return
    d = first_minibatch(fx)
    double = fx.kind == "ddqn"
    assert dq._margin_ok(d, d["xn"]).all(), "an argmax on the next states is a matter of rounding"
    with exact_gamma(fx.meta("gamma")):
        e = dq.evaluate(d, np.float64, double=double)
    quad = (np.abs(e["q"] - e["y"]) < 1).mean()
    g = np.abs(fx.f64("ref64/grad/policy"))
    if fx.case == "dqn":
        assert 0.2 <= quad <= 0.8, "Huber's quadratic branch holds %.2f of the TD errors" % quad
        assert fx["draws/index"].shape == (5, 24)
    elif fx.case == "dqn_clamped":
        assert (g == 1.0).any() and ((g > 0) & (g < 1.0)).any() and g.max() == 1.0
        assert fx["draws/index"].shape == (5, 24)
    else:
        assert fx["draws/index"].shape == (5, 1)      # B = 1: the reference's [B, B, 1] broadcast is the per-row target


# -- runs of the project's learners ---------------------------------------------------------------------------------------------------
class Result:
    def __init__(self):
        self.first_grads, self.first_loss, self.losses, self.norms, self.ckpt, self.training_step = {}, None, [], {}, {}, None

    def meet(self, name, net):
        g = np.concatenate([p.grad.detach().double().cpu().numpy().reshape(-1) for p in net.parameters() if p.grad is not None])
        self.first_grads.setdefault(name, g)
        self.norms.setdefault(name, []).append(float(np.sqrt((g * g).sum())))

    def snapshot(self, tag, nets):
        self.ckpt[tag] = {n: {k: v.detach().double().cpu().numpy() for k, v in net.state_dict().items()} for n, net in nets.items()}

    def series(self, names):
        loss = np.array(self.losses, dtype=np.float64)
        out = {"loss/" + str(n): loss[:, i] for i, n in enumerate(names)}
        out.update({"norm/" + n: np.array(v) for n, v in self.norms.items()})
        return out


def _module(cls, sd, device, *args):
    import torch
    layers = [sd["fc.0.weight"].shape[0], sd["fc.1.weight"].shape[0]]
    net = cls(sd["fc.0.weight"].shape[1], *args, layers)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net.to(device)


def _run_maddpg(fx, res, backend, device, optimizer, soft_tau):
    import torch
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
    N, shared = fx.meta("nb_agents"), bool(fx.meta("shared"))

    def module(name):
        sd = fx.init(name)
        net = DDPGNetworkMLP(sd["net.0.weight"].shape[1], sd["net.4.weight"].shape[0], sd["net.0.weight"].shape[0])
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        return net.to(device)

    n = 1 if shared else N
    actors, critics = [module("actor%d" % k) for k in range(n)], [module("critic%d" % k) for k in range(n)]
    learner = MADDPGLearner(actors[0] if shared else actors, critics[0] if shared else critics, N, fx.meta("lr_actor"), fx.meta("lr_critic"),
                            gamma=fx.meta("gamma"), soft_tau=fx.meta("soft_tau") if soft_tau is None else soft_tau, gumbel_tau=fx.meta("gumbel_tau"),
                            batch_size=fx.meta("batch_size"), buffer_capacity=int(fx["in/state"].shape[0]), backend=backend, optimizer=optimizer,
                            shared=shared)
    nets = {}
    for k in range(n):
        nets.update({"actor%d" % k: learner.actors[k], "critic%d" % k: learner.critics[k], "tgt_actor%d" % k: learner.tgt_actors[k],
                     "tgt_critic%d" % k: learner.tgt_critics[k]})
    to = lambda key: torch.from_numpy(fx[key]).to(device)
    learner.buffer.push(to("in/state"), to("in/action"), to("in/reward"), to("in/next_state"))
    index, noise = to("draws/index"), to("draws/noise")      # [U, N, B], [U, N, B, N + 1, 2]: MADDPGLearner.draws' layout per update
    learner.draws = lambda seed: (index[learner.training_step], noise[learner.training_step][:, :, :N].contiguous(),
                                  noise[learner.training_step][:, :, N].contiguous())
    learner.before_step = lambda lrn, kind, agent: res.meet("%s%d" % (kind, own(fx, agent)), nets["%s%d" % (kind, own(fx, agent))])
    for u in range(index.shape[0]):
        a_loss, c_loss = learner.update(seed=0)
        res.losses.append([float(v) for a in range(N) for v in (c_loss[a], a_loss[a])])
        if u == 0:
            res.snapshot("first", nets)
    return learner, nets


def stated_relation(case):
    """run_case's keyword arguments under which the project's learner computes what the reference's does, where the port leaves the
    reference's text on purpose (each is an entry of that module's docstring):

    maddpg_shared   ``MADDPG.update_target`` (ddpg.py:300-303) calls ``agent.update_target()`` once per entry of ``self.agents``; the
                    two agents' nets are one object, so every target is blended TWICE per update: to <- (1 - tau)^2 to +
                    (1 - (1 - tau)^2) from.  ``MADDPGLearner(shared=True)`` blends once, with its ``soft_tau``: it equals the
                    reference's at soft_tau = 2 tau - tau^2."""
    if case == "maddpg_shared":
        tau = fixture(case).meta("soft_tau")
        return dict(soft_tau=2 * tau - tau * tau)
    return {}


def _run_tarmac(fx, res, backend, device, optimizer):
    """``TarMACPPOLearner`` has no hook before its clips: ``_learner.clip_and_step``, which it calls once per net and minibatch, is
    wrapped for the run (and put back) to meet the pre-clip gradients.  backend="hip" runs the critic's kernels too."""
    import torch
    from mdr_amd import _learner as L
    from mdr_amd.tarmac import TarMACCritic
    from mdr_amd.tarmac_ppo import TarMACPPOLearner
    lay = ppo_layout(fx)
    actor = tarmac_actor(fx, torch.float32)
    actor.attention = "dense" if str(device) == "cpu" else "auto"
    actor = actor.to(device)
    critic = TarMACCritic(fx.meta("nb_agents"), fx.meta("F"), fx.meta("Hc"))
    critic.load_state_dict({k: torch.from_numpy(np.array(fx["init/critic/" + k])) for k in fx.keys("critic")}, strict=True)
    critic = critic.to(device)
    nets = {"actor": actor, "critic": critic}
    learner = TarMACPPOLearner(actor, critic, fx.meta("lr_actor"), fx.meta("lr_critic"), clip_param=fx.meta("clip_param"),
                               max_grad_norm=fx.meta("max_grad_norm"), ppo_update_time=fx.meta("ppo_update_time"),
                               batch_size=fx.meta("batch_size"), backend=backend, optimizer=optimizer, critic_backend=backend)
    index = [[torch.from_numpy(i).to(device) for i in epoch] for epoch in lay["index"]]
    learner.minibatches = lambda n, seed, epoch: index[epoch]
    owner = {id(learner.actor_optimizer): "actor", id(learner.critic_optimizer): "critic"}
    inner_clip, inner_step = L.clip_and_step, learner.step_minibatch

    def clip_and_step(opt, params, max_grad_norm, **kw):
        res.meet(owner[id(opt)], nets[owner[id(opt)]])
        return inner_clip(opt, params, max_grad_norm, **kw)

    def step_minibatch(*args, **kw):
        out = inner_step(*args, **kw)
        res.losses.append([float(out[0]), float(out[1])])
        if len(res.losses) == 1:
            res.snapshot("first", nets)
        return out

    learner.step_minibatch = step_minibatch
    batch = dict(state=torch.from_numpy(lay["state"]).to(device), action=torch.from_numpy(lay["action"]).to(device),
                 a_prob=torch.from_numpy(lay["a_prob"]).to(device), **{"return": torch.from_numpy(lay["Gt32"]).to(device)})
    L.clip_and_step = clip_and_step
    try:
        learner.update(batch, seed=0)
    finally:
        L.clip_and_step = inner_clip
    return learner, nets


def run_case(case, backend, device, optimizer=None, soft_tau=None):
    """The project's learner of ``case`` on the fixture's data and recorded draws -> Result.  ``soft_tau``: MADDPG's blend factor,
    where a test states a relation to the reference's (default: the fixture's)."""
    import torch
    fx = fixture(case)
    optimizer = torch.optim.Adam if optimizer is None else optimizer
    res = Result()
    if fx.kind == "tarmac":
        learner, nets = _run_tarmac(fx, res, backend, device, optimizer)
    elif fx.kind == "maddpg":
        learner, nets = _run_maddpg(fx, res, backend, device, optimizer, soft_tau)
    elif fx.kind in ("ppo", "mappo"):
        from mdr_amd.mappo import MAPPOLearner
        from mdr_amd.ppo import PPOLearner
        from mdr_amd.rollout import ActorMLP, CriticMLP
        lay = ppo_layout(fx)
        actor, critic = _module(ActorMLP, fx.init("actor"), device, 2), _module(CriticMLP, fx.init("critic"), device)
        nets = {"actor": actor, "critic": critic}
        learner = (PPOLearner if fx.kind == "ppo" else MAPPOLearner)(
            actor, critic, fx.meta("lr_actor"), fx.meta("lr_critic"), clip_param=fx.meta("clip_param"), max_grad_norm=fx.meta("max_grad_norm"),
            ppo_update_time=fx.meta("ppo_update_time"), batch_size=fx.meta("batch_size"), backend=backend, optimizer=optimizer)
        index = [[torch.from_numpy(i).to(device) for i in epoch] for epoch in lay["index"]]
        learner.minibatches = lambda n, seed, epoch: index[epoch]
        learner.before_clip = lambda lrn: [res.meet(n, net) for n, net in nets.items()]
        inner = learner.step_minibatch

        def step_minibatch(*args):
            out = inner(*args)
            res.losses.append([float(out[0]), float(out[1])])
            if len(res.losses) == 1:
                res.snapshot("first", nets)
            return out

        learner.step_minibatch = step_minibatch
        batch = dict(state=torch.from_numpy(lay["state"]).to(device), action=torch.from_numpy(lay["action"]).to(device),
                     a_prob=torch.from_numpy(lay["a_prob"]).to(device), **{"return": torch.from_numpy(lay["Gt32"]).to(device)})
        learner.update(batch, seed=0)
    else:
        from mdr_amd.dqn import DQNLearner, QNetworkMLP
        double = fx.kind == "ddqn"
        policy = _module(QNetworkMLP, fx.init("policy"), device, 2)
        # the reference's DDQN never blends its target net (mdr_amd/dqn.py's docstring): soft_update=False reproduces that
        learner = DQNLearner(policy, fx.meta("lr"), gamma=fx.meta("gamma"), tau=fx.meta("tau"), buffer_capacity=int(fx["in/state"].shape[0]),
                             batch_size=fx.meta("batch_size"), double=double, backend=backend, optimizer=optimizer, soft_update=not double)
        nets = {"policy": policy, "target": learner.target_net}
        to = lambda k: torch.from_numpy(fx[k]).to(device)
        learner.buffer.push(to("in/state"), to("in/action"), to("in/reward"), to("in/next_state"))
        index = [torch.from_numpy(np.array(i)).to(device) for i in fx["draws/index"]]
        learner.sample = lambda seed: index[learner.training_step]
        learner.before_step = lambda lrn: res.meet("policy", policy)
        for u in range(len(index)):
            res.losses.append([float(learner.update(seed=0))])
            if u == 0:
                res.snapshot("first", nets)
    res.snapshot("last", nets)
    res.training_step = int(learner.training_step)
    return res


# -- the yardstick --------------------------------------------------------------------------------------------------------------------
def _kept(sd):
    return {k: np.asarray(v).reshape(-1)[rec.ckpt_positions(np.asarray(v).shape)] for k, v in sd.items()}


def d_ref32(fx):
    """{net or series: the reference's own float32 noise}."""
    out = {}
    for net in fx.nets():
        out[net] = max(float(np.abs(fx.checkpoint("ref32", ck, net)[k] - fx.checkpoint("ref64", ck, net)[k]).max())
                       for ck in ("first", "last") for k in fx.keys(net))
    s32, s64 = fx.series("ref32"), fx.series("ref64")
    for name in s64:
        out[name] = float(np.abs(s32[name] - s64[name]).max())
    return out


def distances(fx, res):
    """{net or series: the run's distance to ref64, taken as d_ref32 takes the reference's}."""
    out = {}
    for net in fx.nets():
        out[net] = max(float(np.abs(_kept(res.ckpt[ck][net])[k] - fx.checkpoint("ref64", ck, net)[k]).max())
                       for ck in ("first", "last") for k in fx.keys(net))
    s64, got = fx.series("ref64"), res.series(fx["meta/loss_names"])
    for name in s64:
        assert got[name].shape == s64[name].shape, name
        out[name] = float(np.abs(got[name] - s64[name]).max())
    return out


def ratios(fx, res):
    """{net or series: distance / d_ref32} (0 / 0 counts as 0)."""
    d, got = d_ref32(fx), distances(fx, res)
    return {k: (0.0 if got[k] == 0 else (got[k] / d[k] if d[k] > 0 else float("inf"))) for k in d}


def assert_within(fx, res, label):
    r = ratios(fx, res)
    d, got = d_ref32(fx), distances(fx, res)
    print("%s %s: " % (fx.case, label) + ", ".join("%s %.3g/%.3g=%.2f" % (k, got[k], d[k], r[k]) for k in sorted(r)))
    bad = {k: v for k, v in r.items() if not v <= FACTOR}
    assert not bad, "%s %s: beyond %g x d_ref32: %s" % (fx.case, label, FACTOR, bad)
    assert res.training_step == fx.meta("training_step")
    return r


def first_minibatch_ratios(case, res):
    """{net: (|loss - ref64| / bound, max over elements |grad - ref64| / bound)} of a run's first minibatch."""
    ref = first_minibatch_reference(case)
    out = {}
    for i, (net, r) in enumerate(sorted(ref.items())):
        loss = res.losses[0][r.get("loss_column", i)]
        if "named" in r:      # tarmac_ppo_ref's contract, scaled so that 1 is its limit
            from tests import tarmac_ppo_ref as tp
            err = tp.rel_l2(_named(fixture(case), res.first_grads[net]), r["named"]["grad"])
            out[net] = (float(abs(loss - r["loss"]) / max(tp.FACTOR * r["loss_yard"], tp.FLOOR * abs(r["loss"]))),
                        max(err[n] / max(tp.FACTOR * r["named"]["yard"][n], tp.FLOOR) for n in err))
            continue
        out[net] = (float(abs(loss - r["loss"]) / r["loss_bound"]), pr.worst(res.first_grads[net], r["grad"], r["grad_bound"]))
    return out


def maddpg_actor_grad_ratios(case, res):
    """{actor: max|grad - ref64| / max|ref32 - ref64|} of each actor's first gradient.  The actor's step reads its critic AFTER that
    critic's first Adam step, whose weights are off the dyadic grids: the derived bound's precondition does not hold there, so the
    yardstick is the reference's own float32 distance, as for the parameters (at most FACTOR)."""
    fx = fixture(case)
    out = {}
    for k in range(1 if fx.meta("shared") else fx.meta("nb_agents")):
        name = "actor%d" % k
        g64 = fx.f64("ref64/grad/" + name)
        d = np.abs(fx["ref32/grad/" + name].astype(np.float64) - g64).max()
        out[name] = float(np.abs(res.first_grads[name] - g64).max() / d)
    return out
