"""TarMAC-PPO's centralised critic step (mdr_tarmac_critic_value / mdr_tarmac_critic_grad, include/mdr_policy.h) restated in numpy on
the CPU: the formulas in a chosen dtype and summation order, the fp64 values they must equal, and a per-element rounding bound - in
the manner of tests/ppo_grad_ref.py, whose grids, `forward` and propagation rules are used as they are.  tests/test_tarmac_critic_grad.py
holds the restatement and the bound to account, tests/test_gpu_tarmac_critic_grad.py holds the kernels to them.

TarMAC_Critic (agents/network.py:241-259) on N agents of F features, J = N F, hidden layers of H units, a minibatch of B env-steps
j_i = index[i] out of M stored ones (state [M, N, F], target [M, N]):

    x_i = state[j_i].reshape(J);  z1 = x W1^T + b1, h1 = relu(z1), z2 = h1 W2^T + b2, h2 = relu(z2), V = h2 W3^T + b3      [B, N]
    delta = target[j] - V;  advantage = delta;  term = delta^2;  loss = (sum_ik term) / (B N)       (pow(delta, 2).mean(0).mean(0))
    dV = (-2 delta) inv,  inv = 1 / (B N) (in fp32: the rounded value);  dz2 = relu'(z2) (dV W3),  dz1 = relu'(z1) (dz2 W2)
    dW3 = dV^T h2, db3 = sum dV, dW2 = dz2^T h1, db2 = sum dz2, dW1 = dz1^T x, db1 = sum dz1          (dV carries the scale)

Inputs on ppo_grad_ref's dyadic grids (state k / 4 in [-1, 1], W1 k / 8, W2 k / 64, W3 k / 16, biases k / 32), targets k / 4 in
[-3, 3]: z1 and z2 are exact in fp32 in any summation order at every shape of NETS - at J = 2550 |z1| <= 1275.25 on a grid of 1 / 32,
|z2| <= 64 * 1275.25 / 16 + 1 / 4 on a grid of 1 / 2048: below 2^24 grid steps, which tests/test_tarmac_critic_grad.py asserts - so no
ReLU mask is a matter of rounding.

The bound is derived, never fitted (u = 2^-24, first order in u; ppo_grad_ref's rule: a sum of n products in any order, a final
scaling included, is off by at most (n + 2) u sum |a| |b|; inherited errors propagate through the next product):
  V       E_V = (H2 + 4) u (sum_u |W3| h2 + |b3|)                                   (h2 is exact)
  delta   E_delta = E_V + u |delta|  (= the advantage's);  E_term = 2 |delta| E_delta + u delta^2
  loss    (sum E_term + (B N + 2) u sum term) / (B N)
  dV      E_dV = 2 inv E_delta + 3 u |dV|                                           (the rounded 1 / (B N) and two products)
  dz2     E_dz2 = m2 (sum_k E_dV |W3| + (N + 2) u sum_k |dV| |W3|)                  (a contraction over the N agents)
  dz1     E_dz1 = m1 (sum_u E_dz2 |W2| + (H2 + 2) u sum_u |dz2| |W2|)
  dW, db  sum_r E_dz |in| + (B + 2) u sum_r |dz| |in|   with in = h2 / h1 / x / 1 and dz = dV / dz2 / dz1
"""
import functools

import numpy as np

from tests.ppo_grad_ref import PARAM_NAMES, U, _grid, _mm, forward, param_slices, ratio_to_bound, worst  # noqa: F401

# (N, F, H)
NETS = [(1, 8, 16), (2, 3, 24), (3, 51, 64), (5, 63, 97), (17, 5, 40), (20, 51, 64), (50, 51, 64)]
ROWS = [1, 15, 16, 17, 65]
PARENT_ROWS = 65
KC = 128      # the kernels' widest input chunk
VARIANTS = ("mean_B_only", "sum", "no_factor_2", "adv_sign", "relu0", "target_not_gathered", "w3_reversed", "drop_tail_chunk",
            "drop_outputs_past_16")
FLOAT_KEYS = ("value", "advantage", "loss", "dV", "grad")


@functools.lru_cache(maxsize=None)
def draw(N, F, H, rows=PARENT_ROWS, seed=0):
    """The seeded inputs of `rows` stored env-steps for one shape, float32, read-only."""
    r = np.random.default_rng([seed, 0x7C, N, F, H, rows])
    J = N * F
    d = dict(state=_grid(r, -4, 4, 4, (rows, N, F)), target=_grid(r, -12, 12, 4, (rows, N)),
             W1=_grid(r, -4, 4, 8, (H, J)), b1=_grid(r, -8, 8, 32, H), W2=_grid(r, -4, 4, 64, (H, H)), b2=_grid(r, -8, 8, 32, H),
             W3=_grid(r, -4, 4, 16, (N, H)), b3=_grid(r, -8, 8, 32, N))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    for v in d.values():
        v.setflags(write=False)
    return d


def inputs(B, N, F, H):
    """The first B env-steps of the shape's draw (a draw of its own beyond PARENT_ROWS)."""
    d = draw(N, F, H, rows=max(B, PARENT_ROWS))
    return {k: (v[:B] if k in ("state", "target") else v) for k, v in d.items()}


def _rows(d, index):
    M = d["state"].shape[0]
    return np.arange(M) if index is None else np.asarray(index, dtype=np.int64)


def _net(d, x, variant=None):
    n = dict({k: d[k] for k in PARAM_NAMES}, x=x)
    if variant == "w3_reversed":
        n["W3"] = d["W3"][::-1]
    return n


def evaluate(d, dtype=np.float64, perm=False, variant=None, index=None):
    """-> dict(value, advantage [B, N], loss, dV [B, N], grad [flat, torch's parameter order], z1, z2) evaluated in `dtype`; `perm`
    permutes every contraction; `variant` switches one of the deliberately wrong forms of VARIANTS on; `index`: the env-steps of the
    minibatch (None: all, in order)."""
    dt = dtype
    j = _rows(d, index)
    B, (_, N, F) = len(j), d["state"].shape
    x = np.asarray(d["state"], dtype=dt)[j].reshape(B, N * F)
    if variant == "drop_tail_chunk":
        x = x.copy()
        x[:, (N * F) // KC * KC:] = 0
    fw = forward(_net(d, x, variant), dt, perm)
    W2 = np.asarray(d["W2"], dtype=dt)
    W3 = np.asarray(d["W3"][::-1] if variant == "w3_reversed" else d["W3"], dtype=dt)
    z1, h1, z2, h2, V = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    tgt = np.asarray(d["target"], dtype=dt)[np.arange(B) if variant == "target_not_gathered" else j]
    delta = (V - tgt).astype(dt) if variant == "adv_sign" else (tgt - V).astype(dt)
    count = B if variant == "mean_B_only" else 1 if variant == "sum" else B * N
    inv = dt(1.0 / count)
    dV = ((dt(-1 if variant == "no_factor_2" else -2) * delta).astype(dt) * inv).astype(dt)
    if variant == "drop_outputs_past_16":
        dV[:, 16:] = 0
    o = (lambda k: np.random.default_rng(k + 1).permutation(k)) if perm else (lambda k: None)
    m2 = (z2 >= 0) if variant == "relu0" else (z2 > 0)
    m1 = (z1 >= 0) if variant == "relu0" else (z1 > 0)
    dz2 = (_mm(dV, W3, o(N)) * m2).astype(dt)
    dz1 = (_mm(dz2, W2, o(W2.shape[0])) * m1).astype(dt)
    ob = o(B)
    ones = np.ones((B, 1), dtype=dt)
    g = [_mm(dz1.T, x, ob), _mm(dz1.T, ones, ob), _mm(dz2.T, h1, ob), _mm(dz2.T, ones, ob), _mm(dV.T, h2, ob), _mm(dV.T, ones, ob)]
    term = (delta * delta).astype(dt)
    loss = dt(term.sum(dtype=dt) / dt(count))
    return dict(value=V, advantage=delta, loss=loss, dV=dV, grad=np.concatenate([t.astype(dt).reshape(-1) for t in g]), z1=z1, z2=z2)


def bound(d, index=None):
    """-> dict(value, advantage, loss, dV, grad): the module docstring's bounds, in fp64 on the exact quantities."""
    j = _rows(d, index)
    B, (_, N, F) = len(j), d["state"].shape
    x = np.asarray(d["state"], dtype=np.float64)[j].reshape(B, N * F)
    fw = forward(_net(d, x), np.float64)
    W2, W3, b3 = (np.asarray(d[k], dtype=np.float64) for k in ("W2", "W3", "b3"))
    z1, h1, z2, h2, V = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    H2 = W3.shape[1]
    E_V = (H2 + 4) * U * (h2 @ np.abs(W3).T + np.abs(b3))
    delta = np.asarray(d["target"], dtype=np.float64)[j] - V
    E_delta = E_V + U * np.abs(delta)
    term, E_term = delta * delta, 2 * np.abs(delta) * E_delta + U * delta * delta
    inv = 1.0 / (B * N)
    dV = -2 * delta * inv
    E_dV = 2 * inv * E_delta + 3 * U * np.abs(dV)
    m2, m1 = z2 > 0, z1 > 0
    dz2 = (dV @ W3) * m2
    E_dz2 = m2 * (E_dV @ np.abs(W3) + (N + 2) * U * (np.abs(dV) @ np.abs(W3)))
    dz1 = (dz2 @ W2) * m1
    E_dz1 = m1 * (E_dz2 @ np.abs(W2) + (H2 + 2) * U * (np.abs(dz2) @ np.abs(W2)))
    one = np.ones((B, 1))

    def acc(E_dz, dz, inp):
        return (E_dz.T @ np.abs(inp) + (B + 2) * U * (np.abs(dz).T @ np.abs(inp))).reshape(-1)

    grad = np.concatenate([acc(E_dz1, dz1, x), acc(E_dz1, dz1, one), acc(E_dz2, dz2, h1), acc(E_dz2, dz2, one), acc(E_dV, dV, h2), acc(E_dV, dV, one)])
    return dict(value=E_V, advantage=E_delta, loss=(E_term.sum() + (B * N + 2) * U * term.sum()) * inv, dV=E_dV, grad=grad)


def worst_of(got, ref, bnd, keys=FLOAT_KEYS):
    """The largest |error| / bound over the float outputs named."""
    return max(worst(got[k], ref[k], bnd[k]) for k in keys if k in got)


@functools.lru_cache(maxsize=None)
def reference(B, N, F, H):
    """The inputs, the fp64 values and the bounds of one case, computed once and shared read-only: dict(inputs, ref, bound)."""
    d = inputs(B, N, F, H)
    ref, bnd = evaluate(d), bound(d)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)
