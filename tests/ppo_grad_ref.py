"""PPO's two minibatch losses and their gradients (mdr_ppo_actor_grad / mdr_ppo_critic_grad, include/mdr_policy.h) restated in numpy on
the CPU: the formulas in a chosen dtype and summation order, the fp64 values they must equal, and a per-element rounding bound.
tests/test_ppo_grad.py holds the restatement and the bound to account, tests/test_gpu_ppo_grad.py holds the kernels to them.

Network Linear(F,H1) - ReLU - Linear(H1,H2) - ReLU - Linear(H2,O) (agents/network.py:14-57), minibatch of B rows:

    z1 = x W1^T + b1, h1 = relu(z1), z2 = h1 W2^T + b2, h2 = relu(z2), l = h2 W3^T + b3
    actor  (agents/ppo.py:153-169)   a = action, d = l_a - l_b (b the other action), p_a = 1 / (1 + e^-d), p_b = 1 / (1 + e^d),
           ratio = p_a / old, s1 = ratio A, s2 = clamp(ratio, 1 - clip, 1 + clip) A, term = -min(s1, s2),
           active = (1 - clip <= ratio <= 1 + clip) or s1 < s2, dl_a = active ? -A ratio p_b : 0, dl_b = -dl_a
    critic (agents/ppo.py:148-150, 180)  adv = target - l_0, term = adv^2, dl_0 = -2 adv
    loss = (1 / B) sum term;  dz2 = relu'(z2) (dl W3), dz1 = relu'(z1) (dz2 W2), relu'(z) = [z > 0]
    dW3 = dl^T h2 / B, db3 = sum dl / B, dW2 = dz2^T h1 / B, db2 = sum dz2 / B, dW1 = dz1^T x / B, db1 = sum dz1 / B

Inputs on dyadic grids (state k / 4 in [-1, 1], W1 k / 8 in [-1/2, 1/2], W2 k / 64 in [-1/16, 1/16], W3 k / 16 in [-1/4, 1/4], biases k / 32
in [-1/4, 1/4]) make z1 and z2 exact in fp32 in any summation order, so the ReLU masks are never a matter of rounding; old_prob is
kept 1e-3 away (relative to 1) from the clip bounds, so the gradient rule is not either.  Every case of a network is a PREFIX of one
257-row draw of that network: the statistical conditions the tests assert are asserted on that draw.

The bound is derived, never fitted to what a kernel returns (u = 2^-24, first order in u, every constant rounded up).  A sum of n
products in ANY order (fma chains, a tree across lanes, workgroups, the final scaling) is off by at most (n + 2) u sum |a| |b|; inherited
errors propagate through the next product.
  logits  E_l = (H2 + 4) u (sum_u |W3| h2 + |b3|)                                       (h2 is exact)
  actor   E_d = E_la + E_lb + u |d|;  p_a is off by rel_a = E_d (1 - p_a) + 8 u (dp / dd = p (1 - p); the exponential, the sum, the
          reciprocal), p_b by rel_b = E_d p_a + 8 u;  ratio by rel_r = rel_a + 2 u;  term by max(|s1|, |s2|) (rel_r + 2 u) (the rounded
          clip bounds included);  dl by |dl| (rel_r + rel_b + 3 u)
  critic  E_adv = E_l + u |adv|,  E_term = 2 |adv| E_adv + u adv^2,  E_dl = 2 E_adv
  loss    (sum E_term + (B + 2) u sum |term|) / B
  dz2     E_dz2 = m2 (sum_o E_dl_o |W3_o| + 2 u sum_o |dl_o W3_o|)
  dz1     E_dz1 = m1 (sum_u E_dz2 |W2| + (H2 + 2) u sum_u |dz2| |W2|)
  dW, db  (sum_r E_dz |in| + (B + 2) u sum_r |dz| |in|) / B  with in = h2 / h1 / x / 1 and dz = dl / dz2 / dz1
"""
import functools

import numpy as np

U = 2.0 ** -24
CLIP = 0.2
NETS = [(51, 100, 100), (22, 100, 100), (64, 128, 128), (8, 16, 16), (63, 97, 113)]
ROWS = [1, 15, 16, 17, 33, 64, 65, 257]
PARENT_ROWS = 257
# (B, F, H1, H2): every B with the default network, every network with 65 and 257 rows
SWEEP = [(B,) + NETS[0] for B in ROWS] + [(B,) + net for net in NETS[1:] for B in (65, 257)]
PARAM_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")

VARIANTS_ACTOR = ("no_clip", "max", "adv_sign", "sum", "relu0", "mask2_on_1", "other_action")
VARIANTS_CRITIC = ("no_factor_2",)


def _grid(rng, lo, hi, den, shape):
    return rng.integers(lo, hi + 1, shape) / float(den)


@functools.lru_cache(maxsize=None)
def draw(F, H1, H2, O, rows=PARENT_ROWS, seed=0):
    """The seeded inputs of `rows` transitions for one network and head, float32 / int64, read-only."""
    r = np.random.default_rng([seed, 0x99, F, H1, H2, O, rows])
    d = dict(x=_grid(r, -4, 4, 4, (rows, F)), W1=_grid(r, -4, 4, 8, (H1, F)), b1=_grid(r, -8, 8, 32, H1),
             W2=_grid(r, -4, 4, 64, (H2, H1)), b2=_grid(r, -8, 8, 32, H2), W3=_grid(r, -4, 4, 16, (O, H2)), b3=_grid(r, -8, 8, 32, O))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    if O == 2:
        d["action"] = r.integers(0, 2, rows).astype(np.int64)
        d["adv"] = r.standard_normal(rows).astype(np.float32)
        fw = forward(d, np.float64)
        a = d["action"]
        dd = fw["l"][np.arange(rows), a] - fw["l"][np.arange(rows), 1 - a]
        p = 1.0 / (1.0 + np.exp(-dd))
        old = (p * np.exp(0.3 * r.standard_normal(rows))).astype(np.float32)
        for _ in range(4):      # rows whose ratio sits within 1e-3 of a clip bound move away from it
            ratio = p / old.astype(np.float64)
            close = (np.abs(ratio - (1 - CLIP)) < 1e-3) | (np.abs(ratio - (1 + CLIP)) < 1e-3)
            old = np.where(close, old * np.float32(1.01), old).astype(np.float32)
        d["old"] = old
    else:
        d["target"] = r.standard_normal(rows).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


def inputs(B, F, H1, H2, O):
    """The first B rows of the network's draw (a draw of its own beyond PARENT_ROWS)."""
    d = draw(F, H1, H2, O, rows=max(B, PARENT_ROWS))
    return {k: (v[:B] if k in ("x", "action", "adv", "old", "target") else v) for k, v in d.items()}


def _mm(a, b, order):
    """a [m, k] @ b [k, n] in the arrays' dtype; `order`: None (the library's own blocking) or a permutation of k."""
    if order is None:
        return a @ b
    return a[:, order] @ b[order, :]


def forward(d, dtype, perm=False):
    x, W1, b1, W2, b2, W3, b3 = (np.asarray(d[k], dtype=dtype) for k in ("x", "W1", "b1", "W2", "b2", "W3", "b3"))
    o = (lambda k: np.random.default_rng(k).permutation(k)) if perm else (lambda k: None)
    z1 = (_mm(x, W1.T, o(x.shape[1])) + b1).astype(dtype)
    h1 = np.maximum(z1, 0)
    z2 = (_mm(h1, W2.T, o(h1.shape[1])) + b2).astype(dtype)
    h2 = np.maximum(z2, 0)
    l = (_mm(h2, W3.T, o(h2.shape[1])) + b3).astype(dtype)
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, l=l)


def evaluate(d, dtype=np.float64, perm=False, variant=None, clip=CLIP):
    """-> dict(loss, grad [flat, torch's parameter order], ratio | value, advantage) evaluated in `dtype`; `perm` permutes every
    contraction; `variant` switches one of the deliberately wrong forms of VARIANTS_ACTOR / VARIANTS_CRITIC on."""
    dt = dtype
    fw = forward(d, dt, perm)
    x, W2, W3 = (np.asarray(d[k], dtype=dt) for k in ("x", "W2", "W3"))
    z1, h1, z2, h2, l = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    B = x.shape[0]
    rows = np.arange(B)
    out = {}
    if W3.shape[0] == 2:
        a = d["action"] if variant != "other_action" else 1 - d["action"]
        adv = np.asarray(d["adv"], dtype=dt) * (-1 if variant == "adv_sign" else 1)
        old = np.asarray(d["old"], dtype=dt)
        dd = l[rows, a] - l[rows, 1 - a]
        pa = (1 / (1 + np.exp(-dd))).astype(dt)
        pb = (1 / (1 + np.exp(dd))).astype(dt)
        ratio = (pa / old).astype(dt)
        lo, hi = dt(1 - clip), dt(1 + clip)
        s1 = ratio * adv
        s2 = np.clip(ratio, lo, hi) * adv
        inside = (ratio >= lo) & (ratio <= hi)
        if variant == "no_clip":
            term, active = -s1, np.ones(B, dtype=bool)
        elif variant == "max":
            term, active = -np.maximum(s1, s2), inside | (s1 > s2)
        else:
            term, active = -np.minimum(s1, s2), inside | (s1 < s2)
        da = np.where(active, -adv * ratio * pb, 0).astype(dt)
        dl = np.zeros((B, 2), dtype=dt)
        dl[rows, a] = da
        dl[rows, 1 - a] = -da
        out["ratio"] = ratio
    else:
        adv = (np.asarray(d["target"], dtype=dt) - l[:, 0]).astype(dt)
        term = adv * adv
        dl = ((-1 if variant == "no_factor_2" else -2) * adv)[:, None].astype(dt)
        out["value"], out["advantage"] = l[:, 0], adv
    scale = dt(1) if variant == "sum" else dt(1) / dt(B)
    o = (lambda k: np.random.default_rng(k + 1).permutation(k)) if perm else (lambda k: None)
    m2 = (z2 >= 0) if variant == "relu0" else (z2 > 0)
    m1 = (z1 >= 0) if variant == "relu0" else (z1 > 0)
    if variant == "mask2_on_1":
        m1 = m2
    dz2 = (_mm(dl, W3, None) * m2).astype(dt)
    dz1 = (_mm(dz2, W2, o(W2.shape[0])) * m1).astype(dt)
    ob = o(B)
    g = [_mm(dz1.T, x, ob), dz1.sum(axis=0, dtype=dt), _mm(dz2.T, h1, ob), dz2.sum(axis=0, dtype=dt), _mm(dl.T, h2, ob), dl.sum(axis=0, dtype=dt)]
    out["grad"] = np.concatenate([(t * scale).astype(dt).reshape(-1) for t in g])
    out["loss"] = dt(term.sum(dtype=dt) * scale)
    return out


def bound(d, clip=CLIP):
    """-> dict(loss, grad [flat], ratio | value, advantage): the module docstring's bounds, in fp64 on the exact quantities."""
    fw = forward(d, np.float64)
    x, W2, W3, b3 = (np.asarray(d[k], dtype=np.float64) for k in ("x", "W2", "W3", "b3"))
    z1, h1, z2, h2, l = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    B, H2 = x.shape[0], W3.shape[1]
    rows = np.arange(B)
    E_l = (H2 + 4) * U * (h2 @ np.abs(W3).T + np.abs(b3))
    out = {}
    if W3.shape[0] == 2:
        a = d["action"]
        adv, old = np.asarray(d["adv"], dtype=np.float64), np.asarray(d["old"], dtype=np.float64)
        dd = l[rows, a] - l[rows, 1 - a]
        pa, pb = 1 / (1 + np.exp(-dd)), 1 / (1 + np.exp(dd))
        ratio = pa / old
        s1, s2 = ratio * adv, np.clip(ratio, 1 - clip, 1 + clip) * adv
        active = ((ratio >= 1 - clip) & (ratio <= 1 + clip)) | (s1 < s2)
        da = np.where(active, -adv * ratio * pb, 0)
        E_d = E_l[:, 0] + E_l[:, 1] + U * np.abs(dd)
        rel_a, rel_b = E_d * (1 - pa) + 8 * U, E_d * pa + 8 * U
        rel_r = rel_a + 2 * U
        E_term = np.maximum(np.abs(s1), np.abs(s2)) * (rel_r + 2 * U)
        term = -np.minimum(s1, s2)
        dl = np.zeros((B, 2))
        dl[rows, a], dl[rows, 1 - a] = da, -da
        E_dl = np.repeat((np.abs(da) * (rel_r + rel_b + 3 * U))[:, None], 2, axis=1)
        out["ratio"] = ratio * rel_r
    else:
        adv = np.asarray(d["target"], dtype=np.float64) - l[:, 0]
        E_adv = E_l[:, 0] + U * np.abs(adv)
        term, E_term = adv * adv, 2 * np.abs(adv) * E_adv + U * adv * adv
        dl, E_dl = (-2 * adv)[:, None], (2 * E_adv)[:, None]
        out["value"], out["advantage"] = E_l[:, 0], E_adv
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


def param_slices(F, H1, H2, O):
    sizes = [H1 * F, H1, H2 * H1, H2, O * H2, O]
    off = np.concatenate([[0], np.cumsum(sizes)])
    return {n: slice(int(off[i]), int(off[i + 1])) for i, n in enumerate(PARAM_NAMES)}


def ratio_to_bound(got, ref, bnd):
    """|got - ref| / bound per element (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / bnd)


def worst(got, ref, bnd):
    return float(np.max(ratio_to_bound(got, ref, bnd)))


@functools.lru_cache(maxsize=None)
def reference(B, F, H1, H2, O):
    """The inputs, the fp64 values and the bounds of one case, computed once and shared read-only: dict(inputs, ref, bound)."""
    d = inputs(B, F, H1, H2, O)
    ref, bnd = evaluate(d, np.float64), bound(d)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)
