"""MADDPG's TD target with one target actor PER AGENT (mdr_maddpg_target_agents, include/mdr_policy.h; ddpg.py:282-284) restated in
numpy on tests/maddpg_grad_ref.py's inputs, bounds and rules.

Agent k's target actor is drawn on the same dyadic grids as maddpg_grad_ref's, the seed extended by the agent index; net 0 is the
shared case's own target actor, so N equal nets ARE the shared case.  Everything else of a case - states, rewards, noise, the target
critic - is maddpg_grad_ref's.  The target with per-agent picks:

    next_action[:, k] = pick(tgt_actor_k(next_state[:, k]), noise_t[:, k]);  next_q = tgt_critic(joint(next_state, next_action))
    y = reward[:, a] + gamma next_q

The bounds of y and next_q are maddpg_grad_ref's (`logit_bound`, `t_bound` are used as they are): the critic is one net and the picks
are exact.  Picks within twice the bound - |t_0 - t_1| <= 2 (E_t0 + E_t1), at either tau - get their noise drawn again, at most four
passes, then none may be left: `draw`'s own rule, applied to every agent's own net."""
import functools

import numpy as np

from tests import maddpg_grad_ref as R
from tests.ppo_grad_ref import PARAM_NAMES, _grid, forward

TAUS = (1.0, 0.5)
# the seed of agent k's net is (NET_SEED, maddpg_grad_ref's key, k).  12 is the first seed at which a wrong net shows at EVERY shape
# that has a second net - net 0 and net 1 disagree on 6 - 26 of agent 1's 65 picks (at seed 0 the 3-feature nets of the (2, 3, 16, 24)
# shape agree on all 65: their logit differences are a tenth of the noise) - and no pick is a matter of rounding on the first pass
NET_SEED = 12


@functools.lru_cache(maxsize=None)
def target_actors(N, F, Ha, Hc, equal=False):
    """Agent k's target actor: a tuple of N dicts W1 .. b3 (float32, read-only).  Net 0 (and, with `equal`, every net) is the
    shared case's."""
    shared = R.draw(N, F, Ha, Hc)
    nets = []
    for k in range(N):
        if k == 0 or equal:
            net = {n: shared["t" + n] for n in PARAM_NAMES}
        else:
            r = np.random.default_rng([NET_SEED, 0xDD, N, F, Ha, Hc, R.PARENT_ROWS, k])
            net = dict(W1=_grid(r, -4, 4, 8, (Ha, F)), b1=_grid(r, -8, 8, 32, Ha), W2=_grid(r, -4, 4, 64, (Ha, Ha)), b2=_grid(r, -8, 8, 32, Ha),
                       W3=_grid(r, -4, 4, 16, (2, Ha)), b3=_grid(r, -8, 8, 32, 2))
            net = {n: v.astype(np.float32) for n, v in net.items()}
            for v in net.values():
                v.setflags(write=False)
        nets.append(net)
    return tuple(nets)


def _with_actor(d, net):
    """The case's dict with `net` in the place of the target actor: what maddpg_grad_ref's helpers read under the prefix "t"."""
    return dict(d, **{"t" + n: net[n] for n in PARAM_NAMES})


def pick_bad(d, nets, tau):
    """[B, N] bool: picks of agent k's own target actor on next_state[:, k] that would be a matter of rounding."""
    B, N, F = d["next_state"].shape
    bad = np.zeros((B, N), dtype=bool)
    for k, net in enumerate(nets):
        t, E = R.t_bound(_with_actor(d, net), "t", d["next_state"][:, k, :], d["noise_t"][:, k, :], tau)
        bad[:, k] = np.abs(t[:, 0] - t[:, 1]) <= 2 * (E[:, 0] + E[:, 1])
    return bad


@functools.lru_cache(maxsize=None)
def draw(N, F, Ha, Hc, rows=R.PARENT_ROWS, equal=False):
    """-> (d, nets, first): maddpg_grad_ref's inputs of `rows` env-steps with noise_t redrawn where a per-agent pick would be a matter
    of rounding, the N target actors, and the number of such picks on the first pass."""
    base = R.draw(N, F, Ha, Hc, rows=max(rows, R.PARENT_ROWS))
    d = {k: (v[:rows] if k in R.ROW_KEYS else v) for k, v in base.items()}
    d["noise_t"] = np.array(d["noise_t"])
    nets = target_actors(N, F, Ha, Hc, equal)
    r = np.random.default_rng([1, 0xDD, N, F, Ha, Hc, rows])
    first = None
    for _ in range(4):
        bad = np.zeros((rows, N), dtype=bool)
        for tau in TAUS:
            bad |= pick_bad(d, nets, tau)
        first = int(bad.sum()) if first is None else first
        if not bad.any():
            break
        d["noise_t"][bad] = R._gumbel(r, (int(bad.sum()), 2))
    left = sum(int(pick_bad(d, nets, tau).sum()) for tau in TAUS)
    assert left == 0, "%d picks are still a matter of rounding after four passes" % left
    d["noise_t"].setflags(write=False)
    return d, nets, first


def picks(d, nets, tau, dtype=np.float64):
    """next_action uint8 [B, N]: column k from net k."""
    B, N, F = d["next_state"].shape
    ns = np.asarray(d["next_state"], dtype=dtype)
    na = np.zeros((B, N), dtype=np.uint8)
    for k, net in enumerate(nets):
        l = forward(dict(net, x=ns[:, k, :]), dtype)["l"]
        t = R._ts(l, d["noise_t"][:, k, :], tau, dtype)
        na[:, k] = t[:, 1] > t[:, 0]
    return na


def evaluate(d, nets, agent, tau=1.0, dtype=np.float64):
    """-> dict(next_action, next_q, y) in `dtype`."""
    dt = dtype
    ns = np.asarray(d["next_state"], dtype=dt)
    na = picks(d, nets, tau, dt)
    nq = forward(R._net(d, "tc", R.joint(ns, na)), dt)["l"][:, 0]
    y = (np.asarray(d["reward"][:, agent], dtype=dt) + (dt(R.GAMMA) * nq).astype(dt)).astype(dt)
    return dict(next_action=na, next_q=nq.astype(dt), y=y)


def bound(d, nets, agent, tau=1.0):
    """-> dict(next_q, y): maddpg_grad_ref.bound's target part on the per-agent picks."""
    ref = evaluate(d, nets, agent, tau)
    ns = np.asarray(d["next_state"], dtype=np.float64)
    E_nq = R.logit_bound(d, "tc", R.joint(ns, ref["next_action"]))[:, 0]
    E_y = R.GAMMA * E_nq + 2 * R.U * (np.abs(np.asarray(d["reward"], dtype=np.float64)[:, agent]) + R.GAMMA * np.abs(ref["next_q"]))
    return dict(next_q=E_nq, y=E_y)


@functools.lru_cache(maxsize=None)
def reference(B, N, F, Ha, Hc, agent, tau=1.0, equal=False):
    """One case, computed once and shared read-only: dict(inputs, nets, ref, bound)."""
    d, nets, _ = draw(N, F, Ha, Hc, rows=max(B, R.PARENT_ROWS), equal=equal)
    d = {k: (v[:B] if k in R.ROW_KEYS else v) for k, v in d.items()}
    ref, bnd = evaluate(d, nets, agent, tau), bound(d, nets, agent, tau)
    for t in list(ref.values()) + list(bnd.values()):
        t.setflags(write=False)
    return dict(inputs=d, nets=nets, ref=ref, bound=bnd)
