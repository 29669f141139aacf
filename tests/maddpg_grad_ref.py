"""MADDPG's TD target, critic step and actor step (mdr_maddpg_target / mdr_maddpg_critic_grad / mdr_maddpg_actor_grad,
include/mdr_policy.h) restated in numpy on the CPU: the formulas in a chosen dtype and summation order, the fp64 values they must
equal, and a per-element rounding bound - in the manner of tests/ppo_grad_ref.py and tests/dqn_grad_ref.py, whose network, grids,
`forward` and propagation rules are used as they are.  tests/test_maddpg_grad.py holds the restatement and the bound to account,
tests/test_gpu_maddpg_grad.py holds the kernels to them.

Four networks (actor: W1 .. b3, its target: tW1 .., critic: cW1 .., its target: tcW1 ..), N agents, F features, minibatch of B
env-steps (state, next_state [B, N, F], action, reward [B, N]), noise_t [B, N, 2] for the target actor's picks and noise_a [B, N, 2]
of which the actor step of agent a takes [:, a, :]:

    pick(l, g)   t = (l + g) / tau, h = [t_1 > t_0] (a tie: action 0), p = softmax(t) = (sigma(t_0 - t_1), sigma(t_1 - t_0))
    joint(s, h)  x = s.reshape(B, N F) | onehot(h[:, 0]) | ... | onehot(h[:, N - 1]),   J = N (F + 2)
    target       next_action[:, k] = pick(tgt_actor(next_state[:, k]), noise_t[:, k]);  next_q = tgt_critic(joint(next_state, next_action))
                 y = reward[:, a] + gamma next_q                     (gamma is the ABI's float: the fp32 value of 0.99)
    critic       q = critic(joint(state, action)), delta = q - y, loss = (1 / B) sum delta^2, dl = 2 delta / B
    actor        l = actor(state[:, a]), (h, p) = pick(l, noise_a[:, a]);  Q = critic(joint(state, action with column a := h))
                 loss = -(1 / B) sum Q + pse (1 / (2 B)) sum (l_0^2 + l_1^2);  through the critic with dq = -1 / B:
                 dz2 = relu'(z2) dq W3, dz1 = relu'(z1) (dz2 W2), c_o = dz1 . W1[:, N F + 2 a + o];
                 dl_0 = p_0 p_1 (c_0 - c_1) / tau + pse l_0 / B,  dl_1 = -p_0 p_1 (c_0 - c_1) / tau + pse l_1 / B
    grad         as tests/ppo_grad_ref.py from dl, which carries the 1 / B here (as autograd has it): no scaling behind the sums

Inputs on ppo_grad_ref's dyadic grids (z1, z2 exact in fp32 in any order; the one-hot columns are 0 / 1); reward k / 4 in [-3, 3];
noise drawn with numpy as -log(Exp(1)).  Pick rows, in either actor, whose |t_0 - t_1| is not above twice the sum of the two bounds
E_t get their noise drawn again (at most four passes, `draw` asserts that none is left): no pick is a matter of rounding.

The bound is derived, never fitted (u = 2^-24, first order in u; ppo_grad_ref's rule: a sum of n products in any order is off by at
most (n + 2) u sum |a| |b|, inherited errors propagate through the next product):
  logits  E_l = (H2 + 4) u (sum_u |W3| h2 + |b3|) for any net on exact inputs (h2 is exact)
  pick    E_t = (E_l + u |l + g|) / tau + u |t|    (the add and the divide round once each)
  target  E_nextq = E_l of the target critic;  E_y = gamma E_nextq + 2 u (|reward| + gamma |next_q|)    (as dqn_grad_ref)
  critic  E_q = E_l, E_delta = E_q + E_y + u |delta|, E_term = 2 |delta| E_delta + u delta^2,
          E_dl = 2 E_delta / B + 3 u |dl|    (the rounded 1 / B and two products)
  actor   E_d = E_t0 + E_t1 + u |t_1 - t_0|;  the sigmoid: p_c is off by rel_c = E_d (1 - p_c) + 8 u (ppo_grad_ref's rel_a);
          dq = -1 / B is off by u |dq|;  dz2, dz1 by ppo_grad_ref's rules;  the two-column W1 product:
          E_c = sum_u E_dz1 |W1col| + (H1 + 2) u sum_u |dz1| |W1col|;  E_diff = E_c0 + E_c1 + u |c_0 - c_1|;
          s = p_0 p_1 (c_0 - c_1) / tau:  E_s = |s| (rel_0 + rel_1 + 3 u) + p_0 p_1 E_diff / tau;
          reg_c = pse l_c / B:  E_reg = pse E_l / B + 3 u |reg|;   E_dl = E_s + E_reg + u |dl|
          term = pse (l_0^2 + l_1^2) / 2 - Q:  E_term = E_Q + pse (|l_0| E_l0 + |l_1| E_l1) + 4 u pse (l_0^2 + l_1^2) / 2 + u |term|
  loss    (sum E_term + (B + 2) u sum |term|) / B
  dz2     E_dz2 = m2 (sum_o E_dl_o |W3_o| + 4 u sum_o |dl_o W3_o|);  dz1 = m1 (sum_u E_dz2 |W2| + (H2 + 2) u sum_u |dz2| |W2|)
  dW, db  sum_r E_dz |in| + (B + 2) u sum_r |dz| |in|
"""
import functools

import numpy as np

from tests.ppo_grad_ref import PARAM_NAMES, U, _grid, _mm, forward, param_slices, ratio_to_bound, worst  # noqa: F401

GAMMA = float(np.float32(0.99))
PSE = float(np.float32(1e-3))
# (N, F, Ha, Hc)
NETS = [(1, 8, 16, 16), (2, 3, 16, 24), (3, 51, 100, 100), (5, 63, 97, 113), (20, 51, 256, 256)]
ROWS = [1, 15, 16, 17, 65]
PARENT_ROWS = 65
PREFIXES = ("", "t", "c", "tc")
ROW_KEYS = ("state", "next_state", "action", "reward", "noise_t", "noise_a")
VARIANTS = ("soft", "no_tau", "no_pse", "pse_over_B", "wrong_agent_cols", "wrong_reward", "policy_as_target", "relu0", "sum",
            "stored_action")
FLOAT_KEYS = ("y", "next_q", "q", "closs", "cgrad", "Q", "logits", "aloss", "agrad")


def _net(d, prefix, x):
    return dict({n: d[prefix + n] for n in PARAM_NAMES}, x=x)


def logit_bound(d, prefix, x):
    fw = forward(_net(d, prefix, x), np.float64)
    W3, b3 = (np.asarray(d[prefix + k], dtype=np.float64) for k in ("W3", "b3"))
    return (W3.shape[1] + 4) * U * (fw["h2"] @ np.abs(W3).T + np.abs(b3))


def joint(state, act):
    """[B, N, F] and 0 / 1 [B, N] (any dtype: the soft variant passes probabilities of action 1) -> [B, N (F + 2)]."""
    B, N, _ = state.shape
    a = np.asarray(act, dtype=state.dtype)
    onehot = np.stack([1 - a, a], axis=2).reshape(B, 2 * N)
    return np.concatenate([state.reshape(B, -1), onehot], axis=1)


def _ts(l, g, tau, dt):
    return ((l + np.asarray(g, dtype=dt)).astype(dt) / dt(tau)).astype(dt)


def t_bound(d, prefix, x, g, tau):
    """-> (t in fp64 [rows, 2], E_t [rows, 2])."""
    l = forward(_net(d, prefix, x), np.float64)["l"]
    E_l = logit_bound(d, prefix, x)
    s = l + np.asarray(g, dtype=np.float64)
    t = s / tau
    return t, (E_l + U * np.abs(s)) / tau + U * np.abs(t)


def _pick_bad(d, tau):
    """Rows [B, N] of either pick (the target's on next_state, the actor's on state) whose argmax would be a matter of rounding."""
    B, N, F = d["state"].shape
    bad = []
    for prefix, x, g in (("t", d["next_state"], d["noise_t"]), ("", d["state"], d["noise_a"])):
        t, E = t_bound(d, prefix, x.reshape(B * N, F), g.reshape(B * N, 2), tau)
        bad.append((np.abs(t[:, 0] - t[:, 1]) <= 2 * (E[:, 0] + E[:, 1])).reshape(B, N))
    return bad


def _gumbel(r, shape):
    return (-np.log(r.exponential(size=shape))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def draw(N, F, Ha, Hc, rows=PARENT_ROWS, seed=0, taus=(1.0, 0.5)):
    """The seeded inputs of `rows` env-steps for one shape, float32 / int64, read-only."""
    r = np.random.default_rng([seed, 0xDD, N, F, Ha, Hc, rows])
    J = N * (F + 2)
    d = dict(state=_grid(r, -4, 4, 4, (rows, N, F)), next_state=_grid(r, -4, 4, 4, (rows, N, F)), reward=_grid(r, -12, 12, 4, (rows, N)))
    for p, (K, H, O) in zip(PREFIXES, ((F, Ha, 2), (F, Ha, 2), (J, Hc, 1), (J, Hc, 1))):
        d.update({p + "W1": _grid(r, -4, 4, 8, (H, K)), p + "b1": _grid(r, -8, 8, 32, H), p + "W2": _grid(r, -4, 4, 64, (H, H)),
                  p + "b2": _grid(r, -8, 8, 32, H), p + "W3": _grid(r, -4, 4, 16, (O, H)), p + "b3": _grid(r, -8, 8, 32, O)})
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d["action"] = r.integers(0, 2, (rows, N)).astype(np.int64)
    d["noise_t"], d["noise_a"] = _gumbel(r, (rows, N, 2)), _gumbel(r, (rows, N, 2))
    for _ in range(4):      # picks that would be a matter of rounding at either tau get their noise drawn again
        bad_t = np.zeros((rows, N), dtype=bool)
        bad_a = np.zeros((rows, N), dtype=bool)
        for tau in taus:
            bt, ba = _pick_bad(d, tau)
            bad_t |= bt
            bad_a |= ba
        if not bad_t.any() and not bad_a.any():
            break
        d["noise_t"][bad_t] = _gumbel(r, (int(bad_t.sum()), 2))
        d["noise_a"][bad_a] = _gumbel(r, (int(bad_a.sum()), 2))
    left = sum(int(b.sum()) for tau in taus for b in _pick_bad(d, tau))
    assert left == 0, "%d picks are still a matter of rounding after four passes" % left
    for v in d.values():
        v.setflags(write=False)
    return d


def inputs(B, N, F, Ha, Hc):
    """The first B env-steps of the shape's draw (a draw of its own beyond PARENT_ROWS)."""
    d = draw(N, F, Ha, Hc, rows=max(B, PARENT_ROWS))
    return {k: (v[:B] if k in ROW_KEYS else v) for k, v in d.items()}


def _backward(dl, fw, x, W2, W3, dt, perm, variant):
    """ppo_grad_ref's gradient from dl (which carries the 1 / B) -> (flat grad, dz1)."""
    o = (lambda k: np.random.default_rng(k + 1).permutation(k)) if perm else (lambda k: None)
    z1, h1, z2, h2 = fw["z1"], fw["h1"], fw["z2"], fw["h2"]
    m2 = (z2 >= 0) if variant == "relu0" else (z2 > 0)
    m1 = (z1 >= 0) if variant == "relu0" else (z1 > 0)
    dz2 = (_mm(dl, W3, None) * m2).astype(dt)
    dz1 = (_mm(dz2, W2, o(W2.shape[0])) * m1).astype(dt)
    ob = o(x.shape[0])
    g = [_mm(dz1.T, x, ob), dz1.sum(axis=0, dtype=dt), _mm(dz2.T, h1, ob), dz2.sum(axis=0, dtype=dt), _mm(dl.T, h2, ob), dl.sum(axis=0, dtype=dt)]
    return np.concatenate([t.astype(dt).reshape(-1) for t in g]), dz1


def evaluate(d, agent, tau=1.0, pse=PSE, dtype=np.float64, perm=False, variant=None):
    """-> dict(next_action [uint8 B, N], next_q, y, q, closs, cgrad, Q, logits, aloss, agrad) evaluated in `dtype`; `perm` permutes
    every contraction; `variant` switches one of the deliberately wrong forms of VARIANTS on."""
    dt = dtype
    B, N, F = d["state"].shape
    st, ns = np.asarray(d["state"], dtype=dt), np.asarray(d["next_state"], dtype=dt)
    scale = dt(1) if variant == "sum" else dt(1) / dt(B)
    # target
    pa, pc = ("", "c") if variant == "policy_as_target" else ("t", "tc")
    lt = forward(_net(d, pa, ns.reshape(B * N, F)), dt, perm)["l"]
    tt = _ts(lt, d["noise_t"].reshape(B * N, 2), tau, dt)
    na = (tt[:, 1] > tt[:, 0]).reshape(B, N)
    nq = forward(_net(d, pc, joint(ns, na)), dt, perm)["l"][:, 0]
    ra = (agent + 1) % N if variant == "wrong_reward" else agent
    y = (np.asarray(d["reward"][:, ra], dtype=dt) + (dt(GAMMA) * nq).astype(dt)).astype(dt)
    # critic
    xc = joint(st, d["action"])
    fwc = forward(_net(d, "c", xc), dt, perm)
    cW2, cW3, cW1 = (np.asarray(d["c" + k], dtype=dt) for k in ("W2", "W3", "W1"))
    q = fwc["l"][:, 0]
    delta = (q - y).astype(dt)
    dl = ((dt(2) * delta) * scale).astype(dt)[:, None]
    cgrad, _ = _backward(dl, fwc, xc, cW2, cW3, dt, perm, variant)
    closs = dt((delta * delta).sum(dtype=dt) * scale)
    # actor
    xa = st[:, agent, :]
    fwa = forward(_net(d, "", xa), dt, perm)
    l = fwa["l"]
    t = _ts(l, d["noise_a"][:, agent, :], tau, dt)
    h = t[:, 1] > t[:, 0]
    p1 = (1 / (1 + np.exp(t[:, 0] - t[:, 1]))).astype(dt)
    p0 = (1 / (1 + np.exp(t[:, 1] - t[:, 0]))).astype(dt)
    act = np.array(d["action"], dtype=dt)
    col = (agent + 1) % N if variant == "wrong_agent_cols" else agent
    if variant != "stored_action":
        act[:, col] = p1 if variant == "soft" else h
    xq = joint(st, act)
    fwq = forward(_net(d, "c", xq), dt, perm)
    Q = fwq["l"][:, 0]
    dq = np.full((B, 1), -scale, dtype=dt)
    _, dz1 = _backward(dq, fwq, xq, cW2, cW3, dt, perm, variant)
    c = _mm(dz1, cW1[:, N * F + 2 * col:N * F + 2 * col + 2], None).astype(dt)
    s = ((p0 * p1).astype(dt) * (c[:, 0] - c[:, 1]).astype(dt)).astype(dt)
    if variant != "no_tau":
        s = (s / dt(tau)).astype(dt)
    k = dt(0) if variant == "no_pse" else dt(2 * pse) if variant == "pse_over_B" else dt(pse)
    reg = (k * l * scale).astype(dt)
    dla = np.stack([s + reg[:, 0], reg[:, 1] - s], axis=1).astype(dt)
    aW2, aW3 = (np.asarray(d[n], dtype=dt) for n in ("W2", "W3"))
    agrad, _ = _backward(dla, fwa, xa, aW2, aW3, dt, perm, variant)
    term = (dt(0.5) * k * (l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) - Q).astype(dt)
    aloss = dt(term.sum(dtype=dt) * scale)
    return dict(next_action=na.astype(np.uint8), next_q=nq.astype(dt), y=y, q=q, closs=closs, cgrad=cgrad, Q=Q, logits=l, aloss=aloss,
                agrad=agrad, pick=h.astype(np.uint8))


def _grad_bound(dl, E_dl, fw, x, W2, W3):
    z1, h1, z2, h2 = fw["z1"], fw["h1"], fw["z2"], fw["h2"]
    B, H2 = x.shape[0], W3.shape[1]
    m2, m1 = z2 > 0, z1 > 0
    dz2 = (dl @ W3) * m2
    E_dz2 = m2 * (E_dl @ np.abs(W3) + 4 * U * (np.abs(dl) @ np.abs(W3)))
    dz1 = (dz2 @ W2) * m1
    E_dz1 = m1 * (E_dz2 @ np.abs(W2) + (H2 + 2) * U * (np.abs(dz2) @ np.abs(W2)))
    one = np.ones((B, 1))

    def acc(E_dz, dz, inp):
        return (E_dz.T @ np.abs(inp) + (B + 2) * U * (np.abs(dz).T @ np.abs(inp))).reshape(-1)

    grad = np.concatenate([acc(E_dz1, dz1, x), acc(E_dz1, dz1, one), acc(E_dz2, dz2, h1), acc(E_dz2, dz2, one), acc(E_dl, dl, h2), acc(E_dl, dl, one)])
    return grad, dz1, E_dz1


def bound(d, agent, tau=1.0, pse=PSE):
    """-> dict(y, next_q, q, closs, cgrad, Q, logits, aloss, agrad): the module docstring's bounds, in fp64 on the exact quantities."""
    ref = evaluate(d, agent, tau, pse, np.float64)
    B, N, F = d["state"].shape
    st, ns = np.asarray(d["state"], dtype=np.float64), np.asarray(d["next_state"], dtype=np.float64)
    f64 = lambda k: np.asarray(d[k], dtype=np.float64)      # noqa: E731
    out = {}
    # target
    E_nq = logit_bound(d, "tc", joint(ns, ref["next_action"]))[:, 0]
    E_y = GAMMA * E_nq + 2 * U * (np.abs(f64("reward")[:, agent]) + GAMMA * np.abs(ref["next_q"]))
    out["next_q"], out["y"] = E_nq, E_y
    # critic
    xc = joint(st, d["action"])
    fwc = forward(_net(d, "c", xc), np.float64)
    E_q = logit_bound(d, "c", xc)[:, 0]
    delta = ref["q"] - ref["y"]
    E_delta = E_q + E_y + U * np.abs(delta)
    dl = (2 * delta / B)[:, None]
    E_dl = (2 * E_delta / B)[:, None] + 3 * U * np.abs(dl)
    E_term = 2 * np.abs(delta) * E_delta + U * delta * delta
    out["q"] = E_q
    out["closs"] = (E_term.sum() + (B + 2) * U * (delta * delta).sum()) / B
    out["cgrad"], _, _ = _grad_bound(dl, E_dl, fwc, xc, f64("cW2"), f64("cW3"))
    # actor
    xa = st[:, agent, :]
    fwa = forward(_net(d, "", xa), np.float64)
    l = fwa["l"]
    E_l = logit_bound(d, "", xa)
    t, E_t = t_bound(d, "", xa, d["noise_a"][:, agent, :], tau)
    dd = t[:, 1] - t[:, 0]
    E_d = E_t[:, 0] + E_t[:, 1] + U * np.abs(dd)
    p1, p0 = 1 / (1 + np.exp(-dd)), 1 / (1 + np.exp(dd))
    rel1, rel0 = E_d * (1 - p1) + 8 * U, E_d * (1 - p0) + 8 * U
    act = np.array(d["action"], dtype=np.float64)
    act[:, agent] = ref["pick"]
    xq = joint(st, act)
    fwq = forward(_net(d, "c", xq), np.float64)
    E_Q = logit_bound(d, "c", xq)[:, 0]
    dq = np.full((B, 1), -1.0 / B)
    _, dz1, E_dz1 = _grad_bound(dq, U * np.abs(dq), fwq, xq, f64("cW2"), f64("cW3"))
    W1col = f64("cW1")[:, N * F + 2 * agent:N * F + 2 * agent + 2]
    H1 = W1col.shape[0]
    c = dz1 @ W1col
    E_c = E_dz1 @ np.abs(W1col) + (H1 + 2) * U * (np.abs(dz1) @ np.abs(W1col))
    diff = c[:, 0] - c[:, 1]
    E_diff = E_c[:, 0] + E_c[:, 1] + U * np.abs(diff)
    s = p0 * p1 * diff / tau
    E_s = np.abs(s) * (rel0 + rel1 + 3 * U) + p0 * p1 * E_diff / tau
    reg = pse * l / B
    E_reg = pse * E_l / B + 3 * U * np.abs(reg)
    dla = np.stack([s + reg[:, 0], reg[:, 1] - s], axis=1)
    E_dla = E_s[:, None] + E_reg + U * np.abs(dla)
    sq = 0.5 * pse * (l[:, 0] ** 2 + l[:, 1] ** 2)
    term = sq - ref["Q"]
    E_term = E_Q + pse * (np.abs(l) * E_l).sum(axis=1) + 4 * U * sq + U * np.abs(term)
    out["Q"], out["logits"] = E_Q, E_l
    out["aloss"] = (E_term.sum() + (B + 2) * U * np.abs(term).sum()) / B
    out["agrad"], _, _ = _grad_bound(dla, E_dla, fwa, xa, f64("W2"), f64("W3"))
    return out


def worst_of(got, ref, bnd, keys=FLOAT_KEYS):
    """The largest |error| / bound over the float outputs named."""
    return max(worst(got[k], ref[k], bnd[k]) for k in keys)


@functools.lru_cache(maxsize=None)
def reference(B, N, F, Ha, Hc, agent, tau=1.0):
    """The inputs, the fp64 values and the bounds of one case, computed once and shared read-only: dict(inputs, ref, bound)."""
    d = inputs(B, N, F, Ha, Hc)
    ref, bnd = evaluate(d, agent, tau), bound(d, agent, tau)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)
