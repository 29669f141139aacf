"""What mdr_ppo_actor_grad_bf16x3 / mdr_ppo_critic_grad_bf16x3 compute (include/mdr_policy.h, csrc/mdr_ppo_grad_bf16.hip), restated in
numpy on the CPU: tests/ppo_grad_ref.py's formulas with the five matrix products F1 (x W1^T), F2 (h1 W2^T), B2 (dz2 W2), dW2 = dz2^T h1
and dW1 = dz1^T x as three products of bf16 heads and tails each (tests/tarmac_bf16_ref.split), the wrong variants that drop one cross
term, inputs on grids that make the forward exact in that arithmetic, full-mantissa inputs, and a per-element bound.
tests/test_ppo_grad_bf16.py holds restatement, inputs and bound to account; tests/test_gpu_ppo_grad_bf16.py holds the kernels to them.

The split.  bf16 keeps 8 significand bits.  For a in [2^e, 2^(e+1)): ah = bf16(a) (nearest even) leaves |a - ah| <= 2^(e-8), so the
tail al = bf16(a - ah) has |al| <= 2^-8 |a|, and rounding the residual (< 2^(e-8), or the power of two itself, which is exact) to 8
bits leaves |a - ah - al| <= 2^(e-17) <= 2^-17 |a|.  A product a b taken as ah bh + al bh + ah bl is therefore off by
    al bl + (a - ah - al) b + a (b - bh - bl)   (first order)   <=  (2^-16 + 2^-17 + 2^-17) |a| |b| = 2^-15 |a| |b|
and an operand that is exact in bf16 (no tail) or splits exactly (no residual) drops its terms.  T(l, r) below is that expression
summed over the contraction.  For an operand the test knows exactly (the inputs; h1 on the grid inputs) tail and residual are computed
from its values; for one the kernel computes (h1 on full-mantissa inputs, dz2, dz1) the worst case above stands, on the exact values
(first order).  tests/test_ppo_grad_bf16.py checks the two constants on random values.

The bound (u = 2^-24, first order, every constant rounded up) is ppo_grad_ref.bound's with, for each of the five products,
  - T(l, r) added,
  - the accumulation term of a sum of n products in any order, (n + 2) u sum |a| |b|, taken for the 3 n products it has become:
    (3 n + 2) u sum |a| |b|,
  - inherited errors of both operands propagated (E_l |r| + |l| E_r).
On the grid inputs (`exact_forward=True`) z1 and z2 are exact in this arithmetic in any summation order - the test asserts it - so
E_z1 = E_z2 = 0 as in ppo_grad_ref.bound and h1 is an operand known exactly.  On full-mantissa inputs
    E_z1 = T(x, W1^T) + (3 F + 2) u (|x| |W1|^T + |b1|),   E_z2 = E_z1 |W2|^T + T(h1, W2^T) + (3 H1 + 2) u (h1 |W2|^T + |b2|),
    E_l  = E_z2 |W3|^T + (H2 + 4) u (h2 |W3|^T + |b3|)
and a row in which some unit has |z| <= E_z may take another ReLU mask than fp64: `risky_rows` finds those from the inputs and the
bound alone, the gradient is judged on the others.  Nothing here is fitted to what a kernel returns."""
import functools

import numpy as np

from tests import ppo_grad_ref as pr
from tests.tarmac_bf16_ref import split

U = pr.U
CLIP = pr.CLIP
TAIL, RESID = 2.0 ** -8, 2.0 ** -17      # |al| <= TAIL |a|, |a - ah - al| <= RESID |a|
NETS = pr.NETS
ROWS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 257]
PARENT_ROWS = 257
SWEEP = [(B,) + NETS[0] for B in ROWS] + [(B,) + net for net in NETS[1:] for B in (65, 257)]
PARAM_NAMES = pr.PARAM_NAMES
ROW_KEYS = ("x", "action", "adv", "old", "target")

# (product, term): "lt" drops left-tail x right-head, "rt" left-head x right-tail; left / right as written in the module docstring.
ALL_VARIANTS = tuple((p, t) for p in ("F1", "F2", "B2", "dW2", "dW1") for t in ("lt", "rt"))
# The forward is exact in the split arithmetic only if no product has a tail on both sides (al bl is dropped), so no single grid
# exercises all ten cross terms.  Three kinds of grid inputs, each with the variants that change something on it; together all ten:
#   "w1"  tails in W1 and h1; x, W2 exact in bf16
#   "x"   tails in x and h1; W1, W2 exact in bf16            (x's tail in F1 and in dW1)
#   "w2"  tails in W2; x, W1 and h1 exact in bf16            (W2's tail in F2 and, as W2^T, in B2)
# dz2 and dz1 are full-mantissa in all of them.
VARIANTS = (("F1", "rt"), ("F2", "lt"), ("B2", "lt"), ("dW2", "lt"), ("dW2", "rt"), ("dW1", "lt"))
GRID_VARIANTS = {"w1": VARIANTS,
                 "x": (("F1", "lt"), ("F2", "lt"), ("B2", "lt"), ("dW2", "lt"), ("dW2", "rt"), ("dW1", "lt"), ("dW1", "rt")),
                 "w2": (("F2", "rt"), ("B2", "lt"), ("B2", "rt"), ("dW2", "lt"), ("dW1", "lt"))}
assert set(v for vs in GRID_VARIANTS.values() for v in vs) == set(ALL_VARIANTS)
VARIANT_L2_WL_XH = ("F2", "rt")      # the layer-2 Wl.xh term
# the cases of the two further kinds: (B, F, H1, H2)
SWEEP_KINDS = [(k, c) for k in ("x", "w2") for c in [(B,) + NETS[0] for B in (1, 17, 257)] + [(65,) + net for net in NETS[1:]]]


def _head_inputs(r, d, rows, O):
    """action, advantage, old_prob (kept 1e-3 off the clip bounds) or the target, as ppo_grad_ref.draw makes them."""
    if O == 2:
        d["action"] = r.integers(0, 2, rows).astype(np.int64)
        d["adv"] = r.standard_normal(rows).astype(np.float32)
        fw = pr.forward(d, np.float64)
        a = d["action"]
        dd = fw["l"][np.arange(rows), a] - fw["l"][np.arange(rows), 1 - a]
        p = 1.0 / (1.0 + np.exp(-dd))
        old = (p * np.exp(0.3 * r.standard_normal(rows))).astype(np.float32)
        for _ in range(4):
            ratio = p / old.astype(np.float64)
            close = (np.abs(ratio - (1 - CLIP)) < 1e-3) | (np.abs(ratio - (1 + CLIP)) < 1e-3)
            old = np.where(close, old * np.float32(1.01), old).astype(np.float32)
        d["old"] = old
    else:
        d["target"] = r.standard_normal(rows).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def draw(F, H1, H2, O, rows=PARENT_ROWS, seed=0, kind="w1"):
    """The grid inputs.  Biases k / 32 with |k| <= 8 and W3 = k / 16 with |k| <= 4 in every kind;
    "w1": state in {-1, 0, 1}, W1 = m / 2048 with |m| <= 1024 (head + tail exact, about half with a tail), W2 = k / 64 with |k| <= 4;
    "x":  state = m / 512 with |m| <= 512 (a quarter with a tail), W1 in {-1/4, 0, 1/4}, W2 = k / 64 with |k| <= 4;
    "w2": state in {-1, 0, 1}, W1 = k / 16 with |k| <= 4 (z1 a multiple of 1/32 below 8: h1 exact in bf16), W2 = m / 8192 with
          |m| <= 512 (a quarter with a tail)."""
    r = np.random.default_rng([seed, 0xB16 + ("w1", "x", "w2").index(kind), F, H1, H2, O, rows])
    g = lambda lo, hi, den, shape: (r.integers(lo, hi + 1, shape) / float(den)).astype(np.float32)
    x, W1, W2 = {"w1": ((-1, 1, 1), (-1024, 1024, 2048), (-4, 4, 64)), "x": ((-512, 512, 512), (-1, 1, 4), (-4, 4, 64)),
                 "w2": ((-1, 1, 1), (-4, 4, 16), (-512, 512, 8192))}[kind]
    d = dict(x=g(*x, (rows, F)), W1=g(*W1, (H1, F)), b1=g(-8, 8, 32, H1), W2=g(*W2, (H2, H1)), b2=g(-8, 8, 32, H2),
             W3=g(-4, 4, 16, (O, H2)), b3=g(-8, 8, 32, O))
    return _head_inputs(r, d, rows, O)


def inputs(B, F, H1, H2, O, kind="w1"):
    """The first B rows of the network's grid draw of that kind."""
    d = draw(F, H1, H2, O, kind=kind)
    return {k: (v[:B] if k in ROW_KEYS else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def full_draw(F, H1, H2, O, seed=0, rows=PARENT_ROWS):
    """Full-mantissa inputs: a seeded torch-default-initialised network, states uniform in [-1, 1]."""
    import torch
    torch.manual_seed(1000 * seed + 7 * F + H1 + H2 + O)
    lin = [torch.nn.Linear(F, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, O)]
    r = np.random.default_rng([seed, 0xF011, F, H1, H2, O, rows])
    d = dict(x=r.uniform(-1, 1, (rows, F)).astype(np.float32))
    for i, l in enumerate(lin):
        d["W%d" % (i + 1)] = l.weight.detach().numpy().copy()
        d["b%d" % (i + 1)] = l.bias.detach().numpy().copy()
    return _head_inputs(r, d, rows, O)


def take_rows(d, keep):
    """The inputs restricted to the rows `keep` (indices); the actor's advantage is in minibatch order and is taken with them."""
    return {k: (v[keep] if k in ROW_KEYS else v) for k, v in d.items()}


# ---- the arithmetic
def mm3(l, r, dtype, order=None, drop=None):
    """l [m, k] @ r [k, n] as lh rh + lt rh + lh rt on the float32 values of l and r, every product accumulated in `dtype` over the
    contraction in `order` (None: as the library blocks it); `drop`: "lt" or "rt" leaves that cross term out."""
    lh, lt = (t.astype(dtype) for t in split(np.asarray(l, dtype=np.float32)))
    rh, rt = (t.astype(dtype) for t in split(np.asarray(r, dtype=np.float32)))
    if order is not None:
        lh, lt, rh, rt = lh[:, order], lt[:, order], rh[order, :], rt[order, :]
    out = lh @ rh
    if drop != "lt":
        out = out + lt @ rh
    if drop != "rt":
        out = out + lh @ rt
    return out.astype(dtype)


def forward_split(d, dtype=np.float64, perm=False, variant=None):
    x, W1, b1, W2, b2, W3, b3 = (np.asarray(d[k], dtype=dtype) for k in ("x", "W1", "b1", "W2", "b2", "W3", "b3"))
    o = (lambda k: np.random.default_rng(k).permutation(k)) if perm else (lambda k: None)
    dr = lambda p: variant[1] if variant and variant[0] == p else None
    z1 = (mm3(x, W1.T, dtype, o(x.shape[1]), dr("F1")) + b1).astype(dtype)
    h1 = np.maximum(z1, 0)
    z2 = (mm3(h1, W2.T, dtype, o(h1.shape[1]), dr("F2")) + b2).astype(dtype)
    h2 = np.maximum(z2, 0)
    l = (pr._mm(h2, W3.T, o(h2.shape[1])) + b3).astype(dtype)
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, l=l)


def evaluate(d, dtype=np.float64, perm=False, variant=None, clip=CLIP):
    """ppo_grad_ref.evaluate with the five products split -> dict(loss, grad [flat], ratio | value, advantage)."""
    dt = dtype
    fw = forward_split(d, dt, perm, variant)
    x, W2, W3 = (np.asarray(d[k], dtype=dt) for k in ("x", "W2", "W3"))
    z1, h1, z2, h2, l = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    B = x.shape[0]
    rows = np.arange(B)
    dr = lambda p: variant[1] if variant and variant[0] == p else None
    out = {}
    if W3.shape[0] == 2:
        a = d["action"]
        adv = np.asarray(d["adv"], dtype=dt)
        old = np.asarray(d["old"], dtype=dt)
        dd = l[rows, a] - l[rows, 1 - a]
        pa = (1 / (1 + np.exp(-dd))).astype(dt)
        pb = (1 / (1 + np.exp(dd))).astype(dt)
        ratio = (pa / old).astype(dt)
        lo, hi = dt(1 - clip), dt(1 + clip)
        s1 = ratio * adv
        s2 = np.clip(ratio, lo, hi) * adv
        term, active = -np.minimum(s1, s2), ((ratio >= lo) & (ratio <= hi)) | (s1 < s2)
        da = np.where(active, -adv * ratio * pb, 0).astype(dt)
        dl = np.zeros((B, 2), dtype=dt)
        dl[rows, a] = da
        dl[rows, 1 - a] = -da
        out["ratio"] = ratio
    else:
        adv = (np.asarray(d["target"], dtype=dt) - l[:, 0]).astype(dt)
        term = adv * adv
        dl = (-2 * adv)[:, None].astype(dt)
        out["value"], out["advantage"] = l[:, 0], adv
    scale = dt(1) / dt(B)
    o = (lambda k: np.random.default_rng(k + 1).permutation(k)) if perm else (lambda k: None)
    dz2 = ((dl @ W3) * (z2 > 0)).astype(dt)
    dz1 = (mm3(dz2, W2, dt, o(W2.shape[0]), dr("B2")) * (z1 > 0)).astype(dt)
    ob = o(B)
    g = [mm3(dz1.T, x, dt, ob, dr("dW1")), dz1.sum(axis=0, dtype=dt), mm3(dz2.T, h1, dt, ob, dr("dW2")), dz2.sum(axis=0, dtype=dt),
         pr._mm(dl.T, h2, ob), dl.sum(axis=0, dtype=dt)]
    out["grad"] = np.concatenate([(t * scale).astype(dt).reshape(-1) for t in g])
    out["loss"] = dt(term.sum(dtype=dt) * scale)
    return out


# ---- the bound
def _resid(a, known):
    """(|tail|, |a - head - tail|) of an operand: from its float32 values if the test knows them, the worst case otherwise."""
    a = np.asarray(a, dtype=np.float64)
    if known:
        a32 = a.astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), a), "an operand known exactly is a float32 array"
        h, t = split(a32)
        return np.abs(t.astype(np.float64)), np.abs(a - h.astype(np.float64) - t.astype(np.float64))
    return TAIL * np.abs(a), RESID * np.abs(a)


def split_term(l, r, l_known, r_known):
    """T(l, r): what l @ r loses as lh rh + lt rh + lh rt, per element of the product."""
    lt, le = _resid(l, l_known)
    rt, re = _resid(r, r_known)
    return lt @ rt + le @ np.abs(r) + np.abs(l) @ re


def forward_bound(d, exact_forward):
    """-> (fw, E_z1, E_z2, E_l): the exact fp64 forward and the bounds of z1, z2 (= those of h1, h2) and the logits."""
    fw = pr.forward(d, np.float64)
    x, W1, b1, W2, b2, W3, b3 = (np.asarray(d[k], dtype=np.float64) for k in ("x", "W1", "b1", "W2", "b2", "W3", "b3"))
    h1, h2 = fw["h1"], fw["h2"]
    F, H1, H2 = x.shape[1], W1.shape[0], W2.shape[0]
    if exact_forward:
        E_z1, E_z2 = np.zeros_like(fw["z1"]), np.zeros_like(fw["z2"])
    else:
        E_z1 = split_term(x, W1.T, True, True) + (3 * F + 2) * U * (np.abs(x) @ np.abs(W1).T + np.abs(b1))
        E_z2 = E_z1 @ np.abs(W2).T + split_term(h1, W2.T, False, True) + (3 * H1 + 2) * U * (h1 @ np.abs(W2).T + np.abs(b2))
    E_l = E_z2 @ np.abs(W3).T + (H2 + 4) * U * (h2 @ np.abs(W3).T + np.abs(b3))
    return fw, E_z1, E_z2, E_l


def risky_rows(d):
    """Rows in which some unit's |z| lies within its forward bound of zero (full-mantissa inputs): bool [rows]."""
    fw, E_z1, E_z2, _ = forward_bound(d, False)
    return (np.abs(fw["z1"]) <= E_z1).any(axis=1) | (np.abs(fw["z2"]) <= E_z2).any(axis=1)


def bound(d, exact_forward=True, clip=CLIP):
    """-> dict(loss, grad [flat], ratio | value, advantage): the module docstring's bound against the exact fp64 values."""
    fw, E_z1, E_z2, E_l = forward_bound(d, exact_forward)
    x, W2, W3 = (np.asarray(d[k], dtype=np.float64) for k in ("x", "W2", "W3"))
    z1, h1, z2, h2, l = fw["z1"], fw["h1"], fw["z2"], fw["h2"], fw["l"]
    B, H2 = x.shape[0], W3.shape[1]
    rows = np.arange(B)
    out = {}
    if W3.shape[0] == 2:      # ppo_grad_ref.bound's head, on this E_l
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
    E_dz1 = m1 * (E_dz2 @ np.abs(W2) + split_term(dz2, W2, False, True) + (3 * H2 + 2) * U * (np.abs(dz2) @ np.abs(W2)))
    one = np.ones((B, 1))

    def vec(E_dz, dz, inp, E_inp):      # a product of the vector unit, a bias gradient (inp = ones): fp32 as in ppo_grad_ref
        return ((E_dz.T @ np.abs(inp) + np.abs(dz).T @ E_inp + (B + 2) * U * (np.abs(dz).T @ np.abs(inp))) / B).reshape(-1)

    def mat(E_dz, dz, inp, E_inp, known):      # a weight gradient on the matrix cores
        return ((E_dz.T @ np.abs(inp) + np.abs(dz).T @ E_inp + split_term(dz.T, inp, False, known)
                 + (3 * B + 2) * U * (np.abs(dz).T @ np.abs(inp))) / B).reshape(-1)

    zero = np.zeros((B, 1))
    out["grad"] = np.concatenate([mat(E_dz1, dz1, x, np.zeros_like(x), True), vec(E_dz1, dz1, one, zero),
                                  mat(E_dz2, dz2, h1, E_z1, exact_forward), vec(E_dz2, dz2, one, zero),
                                  vec(E_dl, dl, h2, E_z2), vec(E_dl, dl, one, zero)])
    return out


FORWARD_KEYS = {2: ("loss", "ratio"), 1: ("loss", "value", "advantage")}


@functools.lru_cache(maxsize=None)
def reference(B, F, H1, H2, O, kind="w1"):
    """The grid inputs, the exact fp64 values and the bounds of one case, computed once and shared read-only."""
    d = inputs(B, F, H1, H2, O, kind)
    ref, bnd = pr.evaluate(d, np.float64), bound(d)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)


@functools.lru_cache(maxsize=None)
def full_reference(F, H1, H2, O, seed=0):
    """Full-mantissa inputs of 257 rows: dict(inputs, keep - the rows that are not risky -, fwd_ref / fwd_bound over all rows (the
    fp64 split restatement and the exact fp64 values with the forward part of the bound), kept (inputs, ref, bound of the kept rows))."""
    d = full_draw(F, H1, H2, O, seed)
    keep = np.flatnonzero(~risky_rows(d))
    kd = take_rows(d, keep)
    return dict(inputs=d, keep=keep, fwd_split=evaluate(d, np.float64), fwd_exact=pr.evaluate(d, np.float64), fwd_bound=bound(d, False),
                kept=dict(inputs=kd, ref=pr.evaluate(kd, np.float64), bound=bound(kd, False)))
