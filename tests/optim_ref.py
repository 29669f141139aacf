"""One step of clamp -> norm clip -> Adam -> target blend (mdr_adam_step, include/mdr_policy.h; mdr_amd.optim.FusedAdam) restated in
numpy in fp64 from fp32 inputs, and a per-element rounding bound for what an fp32 evaluation may differ from it - in the manner of
tests/dqn_grad_ref.py.  tests/test_optim.py holds the restatement to torch.optim.Adam + clip_grad_norm_ in float64,
tests/test_gpu_optim.py holds the kernel (and torch's own fp32 step, the yardstick) to the bound.

A network is a list of segments.  `p`, `m`, `v`, `target` are lists of float32 arrays, `g` a list of float32 arrays or None (a dead
segment: skipped entirely, no part of the norm).  With beta1, beta2, eps, lr, tau, max_norm, clamp as Python floats (doubles):

    g      = clip(g, -clamp, clamp)                                              (clamp None: as it is)
    norm   = sqrt(sum over the live segments of g^2);  coef = min(max_norm / (norm + 1e-6), 1);  g = coef g      (max_norm None: coef = 1)
    m'     = beta1 m + (1 - beta1) g;   v' = beta2 v + (1 - beta2) g^2
    p'     = p - (lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
    target'= (1 - tau) target + tau p'                                            (tau None: as it is)

The bound is derived, never fitted: u = 2^-24, first order in u, one u per rounded operation, one u per constant that the kernel
takes as a float rounded from the double (beta, 1 - beta, lr / bc1, sqrt(bc2), eps, tau, 1 - tau, 1e-6), absolute values wherever two
terms may cancel.  sqrt and division are correctly rounded (one u each).  It takes no account of underflow: inputs are zero or
well above 2^-60 in magnitude.

  norm    the sum of squares is over chunks of 1024 consecutive elements of one live segment: per lane 16 fused multiply-adds in a
          row (16 roundings on a growing sum of non-negative terms), 6 levels of the lane butterfly, then the C chunk sums one after
          the other (C - 1 roundings: the first addition is 0 + x).  Every term is non-negative, so each rounding is at most u times
          the final sum:  E_ss = (16 + 6 + C - 1) u ss;  the square root halves a relative error and rounds once:
          E_norm = norm ((21 + C) / 2 + 1) u
  coef    raw = max_norm / (norm + 1e-6): the sum rounds (u), the constant 1e-6 (u of itself, counted against the sum), the
          division rounds (u):  rel = E_norm / (norm + 1e-6) + 3 u.  min(., 1) is 1-Lipschitz and exact:  E_coef = min(raw, 1) rel
          - and 0 where raw (1 - rel) >= 1: both evaluations take exactly 1
  g       E_g = |g| E_coef + u |coef g|      (one product; 0 without a clip: coef = 1 multiplies exactly)
  m'      each term: constant and product (2 u), the sum once:  E_m = 2 u (beta1 |m| + (1 - beta1) |g|) + (1 - beta1) E_g + u |m'|
  v'      g^2: E_gg = 2 |g| E_g + u g^2;  E_v = 2 u beta2 |v| + (1 - beta2) (E_gg + 2 u g^2) + u |v'|
  p'      s = sqrt(v'): E_s = E_v / (2 s) + u s (0 where v' = 0);  d = s / c2 + eps: E_d = E_s / c2 + 2 u s / c2 + u eps + u d;
          q = m' / d: E_q = E_m / d + |m'| E_d / d^2 + u |q|;  step = a q: E_step = a E_q + 2 u |a q|;  E_p = E_step + u |p'|
  target' E_t = 2 u (1 - tau) |target| + tau E_p + 2 u tau |p'| + u |target'|
"""
import numpy as np

U = 2.0 ** -24
CHUNK = 1024
BETAS, EPS = (0.9, 0.999), 1e-8


def _f64(xs):
    return [None if x is None else np.asarray(x, dtype=np.float64) for x in xs]


def nb_chunks(g):
    return sum(-(-x.size // CHUNK) for x in g if x is not None)


def _prepare(g, max_norm, clamp):
    """-> (clamped g [fp64, None where dead], norm, raw coef or None)."""
    g = _f64(g)
    if clamp is not None:
        g = [None if x is None else np.clip(x, -clamp, clamp) for x in g]
    norm = float(np.sqrt(sum(float((x * x).sum()) for x in g if x is not None)))
    raw = None if max_norm is None else max_norm / (norm + 1e-6)
    return g, norm, raw


def step(p, g, m, v, t, lr, target=None, tau=None, max_norm=None, clamp=None, betas=BETAS, eps=EPS):
    """-> dict(p, m, v, target [lists of fp64 arrays; a dead segment's are its inputs], total_norm): the step in fp64."""
    beta1, beta2 = betas
    p, m, v = _f64(p), _f64(m), _f64(v)
    target = _f64(target) if target is not None else None
    g, norm, raw = _prepare(g, max_norm, clamp)
    coef = 1.0 if raw is None else min(raw, 1.0)
    a, c2 = lr / (1.0 - beta1 ** t), np.sqrt(1.0 - beta2 ** t)
    out = dict(p=[], m=[], v=[], target=[] if target is not None else None, total_norm=norm)
    for i, x in enumerate(g):
        if x is None:
            pn, mn, vn, tn = p[i], m[i], v[i], (target[i] if target is not None else None)
        else:
            x = coef * x
            mn = beta1 * m[i] + (1.0 - beta1) * x
            vn = beta2 * v[i] + (1.0 - beta2) * x * x
            pn = p[i] - a * (mn / (np.sqrt(vn) / c2 + eps))
            tn = None
            if target is not None:
                tn = (1.0 - tau) * target[i] + tau * pn if tau is not None else target[i]
        out["p"].append(pn), out["m"].append(mn), out["v"].append(vn)
        if target is not None:
            out["target"].append(tn)
    return out


def bound(p, g, m, v, t, lr, target=None, tau=None, max_norm=None, clamp=None, betas=BETAS, eps=EPS):
    """-> (step(...), dict(p, m, v, target, total_norm)): the fp64 values and the module docstring's bounds on them (0 for a dead
    segment).  `clamp` and `max_norm` are values a float holds exactly."""
    beta1, beta2 = betas
    ref = step(p, g, m, v, t, lr, target, tau, max_norm, clamp, betas, eps)
    p, m, v = _f64(p), _f64(m), _f64(v)
    target = _f64(target) if target is not None else None
    g, norm, raw = _prepare(g, max_norm, clamp)
    C = nb_chunks(g)
    E_norm = norm * ((21 + C) / 2.0 + 1.0) * U
    coef, E_coef = 1.0, 0.0
    if raw is not None:
        rel = E_norm / (norm + 1e-6) + 3 * U
        coef = min(raw, 1.0)
        E_coef = 0.0 if raw * (1.0 - rel) >= 1.0 else coef * rel
    a, c2 = lr / (1.0 - beta1 ** t), np.sqrt(1.0 - beta2 ** t)
    out = dict(p=[], m=[], v=[], target=[] if target is not None else None, total_norm=E_norm)
    for i, x in enumerate(g):
        if x is None:
            z = np.zeros_like(p[i])
            out["p"].append(z), out["m"].append(z), out["v"].append(z)
            if target is not None:
                out["target"].append(z)
            continue
        mn, vn, pn = ref["m"][i], ref["v"][i], ref["p"][i]
        xs = coef * x
        E_g = np.abs(x) * E_coef + (U * np.abs(xs) if raw is not None else 0.0)
        E_m = 2 * U * (beta1 * np.abs(m[i]) + (1 - beta1) * np.abs(xs)) + (1 - beta1) * E_g + U * np.abs(mn)
        E_gg = 2 * np.abs(xs) * E_g + U * xs * xs
        E_v = 2 * U * beta2 * np.abs(v[i]) + (1 - beta2) * (E_gg + 2 * U * xs * xs) + U * np.abs(vn)
        s = np.sqrt(vn)
        E_s = np.where(s > 0, E_v / (2 * np.where(s > 0, s, 1.0)), 0.0) + U * s
        d = s / c2 + eps
        E_d = E_s / c2 + 2 * U * s / c2 + U * eps + U * d
        q = mn / d
        E_q = E_m / d + np.abs(mn) * E_d / (d * d) + U * np.abs(q)
        E_p = a * E_q + 2 * U * np.abs(a * q) + U * np.abs(pn)
        out["p"].append(E_p), out["m"].append(E_m), out["v"].append(E_v)
        if target is not None:
            if tau is None:
                out["target"].append(np.zeros_like(pn))
            else:
                out["target"].append(2 * U * (1 - tau) * np.abs(target[i]) + tau * E_p + 2 * U * tau * np.abs(pn) + U * np.abs(ref["target"][i]))
    return ref, out


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over the lists (or scalars) of one quantity; an element off with a zero bound gives inf."""
    if not isinstance(ref, (list, tuple)):
        got, ref, bnd = [got], [ref], [bnd]
    worst = 0.0
    for a, r, b in zip(got, ref, bnd):
        err = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(r, dtype=np.float64)).reshape(-1)
        b = np.broadcast_to(np.asarray(b, dtype=np.float64), np.asarray(r).shape).reshape(-1)
        if err.size == 0:
            continue
        ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1.0))
        ratio = np.where((err > 0) & (b <= 0), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
    return worst


# the segment shapes of the cases (the issue's): F = 5, H = 7 / 9, 2 outputs - the first bias starts at float 35 of a flat gradient
SIX = [(7, 5), (7,), (9, 7), (9,), (2, 9), (2,)]
CASES = {
    "six": SIX,
    "ragged": [(3 * CHUNK + 5,)],
    "twenty": [(5, 3), (5,), (5, 5), (5,), (5, 9), (5,), (2, 5), (2,), (5, 5), (5,), (3, 5), (3,), (5, 5), (5,), (4, 5), (4,), (5, 5), (5,),
               (3, 5), (3,)],
    "ones": [(1,)] * 32,
}


def draw(shapes, seed, scale=1.0):
    """Seeded float32 arrays of the shapes: normal, times `scale`."""
    r = np.random.default_rng([seed, len(shapes)])
    return [(r.standard_normal(s) * scale).astype(np.float32) for s in shapes]
