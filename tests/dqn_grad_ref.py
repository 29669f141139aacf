"""DQN's / DDQN's TD target, Huber loss and clamped gradient (mdr_dqn_target / mdr_dqn_grad, include/mdr_policy.h) restated in numpy on
the CPU: the formulas in a chosen dtype and summation order, the fp64 values they must equal, and a per-element rounding bound - in the
manner of tests/ppo_grad_ref.py, whose network, grids, `forward` and propagation rules are used as they are.
tests/test_dqn_grad.py holds the restatement and the bound to account, tests/test_gpu_dqn_grad.py holds the kernels to them.

Two networks of the same shape (policy: W1 .. b3, target: tW1 .. tb3), minibatch of B transitions (x, action, reward, xn):

    target (agents/dqn.py:96-99)     Qt = target(xn);  DQN: next_action = [Qt1 > Qt0], next_q = max(Qt0, Qt1)
           (agents/dqn.py:129-135)   DDQN: next_action = [Qp1 > Qp0] with Qp = policy(xn), next_q = Qt[next_action]   (per row)
                                     y = reward + gamma next_q      (gamma is the ABI's float: the fp32 value of 0.99)
    loss   (agents/dqn.py:93, 102-103)   q = policy(x)[action], delta = q - y, term = |delta| < 1 ? delta^2 / 2 : |delta| - 1 / 2,
                                     dl_action = clip(delta, -1, 1), dl_other = 0;  loss = (1 / B) sum term
    grad   as tests/ppo_grad_ref.py from dl, then clip(grad, -clamp, clamp) element by element (agents/dqn.py:108-109)

Inputs on ppo_grad_ref's dyadic grids (z1, z2 exact in fp32 in any order); reward k / 4 in [-3, 3], so that delta > 1, delta < -1 and
|delta| < 1 all occur often.  After the draw the second output bias of each net is moved (on the k / 32 grid) to the median of
Q0 - Q1 on the next states without it, so that both actions are the maximum about equally often; next-state rows on which either net's
|Q0 - Q1| is not above twice the sum of its two logit bounds are redrawn (at most four passes): no argmax is a matter of rounding.
Every case of a network is a PREFIX of one 257-row draw of that network.

The bound is derived, never fitted (u = 2^-24, first order in u; ppo_grad_ref's rules for sums of products):
  logits  E_l = (H2 + 4) u (sum_u |W3| h2 + |b3|) for either net on either input
  target  max and the gather pass the incoming error through (max is 1-Lipschitz in the larger of the two errors):
          E_nextq = max(E_lt0, E_lt1) (DQN) or E_lt[next_action] (DDQN);  E_y = gamma E_nextq + 2 u (|reward| + gamma |next_q|)
          (the product and the sum round once each)
  loss    E_q = E_l[action], E_delta = E_q + E_y + u |delta|;  the clipped gradient is 1-Lipschitz: E_dl = E_delta;
          E_term = max(|delta|, 1) E_delta + 2 u term
  loss, dz2, dz1, dW, db exactly as tests/ppo_grad_ref.py;  the clamp is 1-Lipschitz and adds nothing.
"""
import functools

import numpy as np

from tests.ppo_grad_ref import NETS, PARAM_NAMES, PARENT_ROWS, ROWS, U, _grid, _mm, forward, param_slices, ratio_to_bound, worst  # noqa: F401

GAMMA = float(np.float32(0.99))
SWEEP = [(B,) + NETS[0] for B in ROWS] + [(B,) + net for net in NETS[1:] for B in (65, 257)]
TARGET_NAMES = tuple("t" + n for n in PARAM_NAMES)
ROW_KEYS = ("x", "xn", "action", "reward")
VARIANTS = ("mse", "huber_no_half", "min_target", "no_gamma", "policy_as_target", "other_action", "both_logits", "no_clamp", "dqn_for_ddqn",
            "sum", "relu0")


def _net(d, target, x):
    """The dict `forward` takes: one of the two parameter sets on the rows `x`."""
    return dict({n: d[("t" if target else "") + n] for n in PARAM_NAMES}, x=x)


def logit_bound(d, target, x):
    fw = forward(_net(d, target, x), np.float64)
    W3, b3 = (np.asarray(d[("t" if target else "") + k], dtype=np.float64) for k in ("W3", "b3"))
    return (W3.shape[1] + 4) * U * (fw["h2"] @ np.abs(W3).T + np.abs(b3))


def _margin_ok(d, xn):
    ok = np.ones(xn.shape[0], dtype=bool)
    for target in (False, True):
        l = forward(_net(d, target, xn), np.float64)["l"]
        E = logit_bound(d, target, xn)
        ok &= np.abs(l[:, 0] - l[:, 1]) > 2 * (E[:, 0] + E[:, 1])
    return ok


@functools.lru_cache(maxsize=None)
def draw(F, H1, H2, rows=PARENT_ROWS, seed=0):
    """The seeded inputs of `rows` transitions for one network shape, float32 / int64, read-only."""
    r = np.random.default_rng([seed, 0xD0, F, H1, H2, rows])
    d = dict(x=_grid(r, -4, 4, 4, (rows, F)), xn=_grid(r, -4, 4, 4, (rows, F)))
    for t in ("", "t"):
        d.update({t + "W1": _grid(r, -4, 4, 8, (H1, F)), t + "b1": _grid(r, -8, 8, 32, H1), t + "W2": _grid(r, -4, 4, 64, (H2, H1)),
                  t + "b2": _grid(r, -8, 8, 32, H2), t + "W3": _grid(r, -4, 4, 16, (2, H2)), t + "b3": _grid(r, -8, 8, 32, 2)})
    d["reward"] = _grid(r, -12, 12, 4, rows)
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d["action"] = r.integers(0, 2, rows).astype(np.int64)
    for target in (False, True):      # both actions the maximum on the next states about equally often
        b3 = d[("t" if target else "") + "b3"]
        l = forward(_net(d, target, d["xn"]), np.float64)["l"] - b3.astype(np.float64)
        b3[1] = b3[0] + np.float32(np.round(np.median(l[:, 0] - l[:, 1]) * 32) / 32)
    for _ in range(4):      # next-state rows whose argmax would be a matter of rounding are drawn again
        bad = ~_margin_ok(d, d["xn"])
        if not bad.any():
            break
        d["xn"][bad] = _grid(r, -4, 4, 4, (int(bad.sum()), F)).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


def inputs(B, F, H1, H2, clamp=np.inf):
    """The first B rows of the network's draw (a draw of its own beyond PARENT_ROWS), `clamp` with them."""
    d = draw(F, H1, H2, rows=max(B, PARENT_ROWS))
    out = {k: (v[:B] if k in ROW_KEYS else v) for k, v in d.items()}
    out["clamp"] = float(clamp)
    return out


def _target(d, dt, perm, variant, double):
    """-> next_action (bool), next_q, y in `dt`."""
    xn = d["xn"]
    rows = np.arange(xn.shape[0])
    Qt = forward(_net(d, variant != "policy_as_target", xn), dt, perm)["l"]
    if double and variant != "dqn_for_ddqn":
        Qp = forward(_net(d, False, xn), dt, perm)["l"]
        na = Qp[:, 1] > Qp[:, 0]
        nq = Qt[rows, na.astype(np.int64)]
    else:
        na = Qt[:, 1] > Qt[:, 0]
        nq = np.minimum(Qt[:, 0], Qt[:, 1]) if variant == "min_target" else np.maximum(Qt[:, 0], Qt[:, 1])
    gamma = dt(1) if variant == "no_gamma" else dt(GAMMA)
    y = (np.asarray(d["reward"], dtype=dt) + (gamma * nq).astype(dt)).astype(dt)
    return na, nq.astype(dt), y


def _head(d, dt, perm, variant, y):
    """-> forward of the policy net on x, q, delta, term, dl [B, 2]."""
    fw = forward(_net(d, False, d["x"]), dt, perm)
    B = d["x"].shape[0]
    rows = np.arange(B)
    a = d["action"] if variant != "other_action" else 1 - d["action"]
    q = fw["l"][rows, a]
    delta = (q - y).astype(dt)
    ad = np.abs(delta)
    if variant == "mse":
        term, dq = delta * delta, 2 * delta
    elif variant == "huber_no_half":
        term, dq = np.where(ad < 1, delta * delta, 2 * ad - 1), 2 * np.clip(delta, -1, 1)
    else:
        term, dq = np.where(ad < 1, dt(0.5) * delta * delta, ad - dt(0.5)), np.clip(delta, -1, 1)
    dl = np.zeros((B, 2), dtype=dt)
    dl[rows, a] = dq
    if variant == "both_logits":
        dl[rows, 1 - a] = dq
    return fw, q, delta, term.astype(dt), dl


def evaluate(d, dtype=np.float64, perm=False, variant=None, double=False):
    """-> dict(y, next_q, next_action [uint8], q, loss, grad [flat, torch's parameter order, clamped at d["clamp"]]) evaluated in
    `dtype`; `perm` permutes every contraction; `variant` switches one of the deliberately wrong forms of VARIANTS on."""
    dt = dtype
    na, nq, y = _target(d, dt, perm, variant, double)
    fw, q, delta, term, dl = _head(d, dt, perm, variant, y)
    x, W2, W3 = (np.asarray(d[k], dtype=dt) for k in ("x", "W2", "W3"))
    z1, h1, z2, h2 = fw["z1"], fw["h1"], fw["z2"], fw["h2"]
    B = x.shape[0]
    scale = dt(1) if variant == "sum" else dt(1) / dt(B)
    o = (lambda k: np.random.default_rng(k + 1).permutation(k)) if perm else (lambda k: None)
    m2 = (z2 >= 0) if variant == "relu0" else (z2 > 0)
    m1 = (z1 >= 0) if variant == "relu0" else (z1 > 0)
    dz2 = (_mm(dl, W3, None) * m2).astype(dt)
    dz1 = (_mm(dz2, W2, o(W2.shape[0])) * m1).astype(dt)
    ob = o(B)
    g = [_mm(dz1.T, x, ob), dz1.sum(axis=0, dtype=dt), _mm(dz2.T, h1, ob), dz2.sum(axis=0, dtype=dt), _mm(dl.T, h2, ob), dl.sum(axis=0, dtype=dt)]
    grad = np.concatenate([(t * scale).astype(dt).reshape(-1) for t in g])
    if variant != "no_clamp":
        grad = np.clip(grad, dt(-d["clamp"]), dt(d["clamp"]))
    return dict(y=y, next_q=nq, next_action=na.astype(np.uint8), q=q, loss=dt(term.sum(dtype=dt) * scale), grad=grad)


def bound(d, double=False):
    """-> dict(y, next_q, q, loss, grad [flat]): the module docstring's bounds, in fp64 on the exact quantities."""
    na, nq, y = _target(d, np.float64, False, None, double)
    fw, q, delta, term, dl = _head(d, np.float64, False, None, y)
    x, W2, W3 = (np.asarray(d[k], dtype=np.float64) for k in ("x", "W2", "W3"))
    z1, h1, z2, h2 = fw["z1"], fw["h1"], fw["z2"], fw["h2"]
    B, H2 = x.shape[0], W3.shape[1]
    rows = np.arange(B)
    E_lt = logit_bound(d, True, d["xn"])
    E_nextq = E_lt[rows, na.astype(np.int64)] if double else E_lt.max(axis=1)
    E_y = GAMMA * E_nextq + 2 * U * (np.abs(np.asarray(d["reward"], dtype=np.float64)) + GAMMA * np.abs(nq))
    E_q = logit_bound(d, False, d["x"])[rows, d["action"]]
    E_delta = E_q + E_y + U * np.abs(delta)
    E_dl = np.zeros((B, 2))
    E_dl[rows, d["action"]] = E_delta
    E_term = np.maximum(np.abs(delta), 1) * E_delta + 2 * U * term
    out = dict(y=E_y, next_q=E_nextq, q=E_q)
    out["loss"] = (E_term.sum() + (B + 2) * U * np.abs(term).sum()) / B
    m2, m1 = z2 > 0, z1 > 0
    dz2 = (dl @ W3) * m2
    E_dz2 = m2 * (E_dl @ np.abs(W3) + 2 * U * (np.abs(dl) @ np.abs(W3)))
    dz1 = (dz2 @ W2) * m1
    E_dz1 = m1 * (E_dz2 @ np.abs(W2) + (H2 + 2) * U * (np.abs(dz2) @ np.abs(W2)))
    one = np.ones((B, 1))

    def acc(E_dz, dz, inp):
        return ((E_dz.T @ np.abs(inp) + (B + 2) * U * (np.abs(dz).T @ np.abs(inp))) / B).reshape(-1)

    out["grad"] = np.concatenate([acc(E_dz1, dz1, x), acc(E_dz1, dz1, one), acc(E_dz2, dz2, h1), acc(E_dz2, dz2, one),
                                  acc(E_dl, dl, h2), acc(E_dl, dl, one)])
    return out


def median_clamp(d, double=False):
    """The clamp case's c: the median of the fp64 |grad| without a clamp, rounded to the float the ABI takes."""
    return float(np.float32(np.median(np.abs(evaluate(dict(d, clamp=np.inf), np.float64, double=double)["grad"]))))


@functools.lru_cache(maxsize=None)
def reference(B, F, H1, H2, double=False, clamp=np.inf):
    """The inputs, the fp64 values and the bounds of one case, computed once and shared read-only: dict(inputs, ref, bound).
    clamp="median": the clamp case."""
    d = inputs(B, F, H1, H2)
    if clamp == "median":
        d["clamp"] = median_clamp(d, double)
    elif clamp != np.inf:
        d["clamp"] = float(clamp)
    ref, bnd = evaluate(d, np.float64, double=double), bound(d, double)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)
