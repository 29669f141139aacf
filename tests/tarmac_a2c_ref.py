"""TarMAC A2C (mdr_tarmac_a2c_forward / _comm / _grad, include/mdr_policy.h; mdr_amd.tarmac_a2c) restated in numpy on the CPU: the
formulas in a chosen dtype and summation order, the fp64 values they must equal, and a per-element rounding bound - in the manner of
tests/ppo_grad_ref.py and tests/tarmac_critic_ref.py, whose grids, `_mm` and `worst` are used as they are.  tests/test_tarmac_a2c.py
holds the restatement and the bound to account, tests/test_gpu_tarmac_a2c_*.py hold the kernels to them.

MultiAgentPolicy (agents/tarmac/model.py:132-266) as A2C_ACKTR builds it (no GRU, one hop) on N agents, F features, C message
floats, S state units, K key units; a minibatch of B env-steps j_i = index[i] out of M stored ones, rows r = (b, n), R = B N:

    in = [obs | comm];  z1 = in W1^T + b1, h1 = leaky(z1);  x = h1 W2^T + b2;  logits = x Wd^T                       (no bias)
    xbar_b = (sum_n x_bn) / N;  m = xbar Wc1^T + bc1, a = leaky(m);  V_b = a . Wc2 + bc2                  (one value per env-step)
    q = x Wq^T + bq, k = x Wk^T + bk, v = x Wv^T + bv;  s_ij = (q_i . k_j) / sqrt(C);  attn = softmax_j over ALL j of the env-step,
    j = i included;  comm_out = attn v
    delta_bn = ret[j]_n - V_b;  d = l_taken - l_other, t = exp(-|d|), (p_taken, p_other) = (1, t) / (1 + t) by the sign of d,
    spn = softplus(-d) = max(-d, 0) + log1p(t) = -log p_taken,  spp = softplus(d) = -log p_other,  H = p_taken spn + p_other spp
    value_loss = sum delta^2 / R;  action_loss = sum delta spn / R (delta detached);  entropy = sum H / R
    loss = vc value_loss + action_loss - ec entropy
    g = inv p_other (ec p_taken d - delta) = d loss / d l_taken, d loss / d l_other = -g    (dH / dl_k = -p_k (log p_k + H), and
    log p_taken + H = p_other d);  inv = 1 / R;  dV_b = cv sum_n delta_bn, cv = -2 vc / R;  da = (dV Wc2) leaky'(m);
    dxbar = da Wc1;  dx_bn = dl_bn Wd + dxbar_b / N;  dz1 = leaky'(z1) (dx W2);  leaky'(z) = 1 for z > 0, 0.01 otherwise
    dW1 = dz1^T in, db1 = sum dz1, dW2 = dx^T h1, db2 = sum dx, dWc1 = da^T xbar, dbc1 = sum da, dWc2 = dV^T a, dbc2 = sum dV,
    dWd = dl^T x - the nine tensors evaluate_actions reaches, in parameters() order; the comm tensors get none.

Inputs on dyadic grids (obs, comm k / 4 in [-1, 1], W1 k / 8, biases k / 32): z1 is exact in fp32 in any order (at most 160 products
on a grid of 1 / 32, |z1| <= 80.25: far below 2^24 grid steps; tests/test_tarmac_a2c.py asserts it), so the first LeakyReLU mask is
never a matter of rounding - and z1 = 0 occurs, which is what tells leaky'(0) = 0.01 from 1.  The slope 0.01 is not dyadic, so
everything behind h1 is inexact and the critic's mask is decided by an inexact m: a case is ADMITTED only if every |m| in fp64
exceeds 8 E_m (`admitted`); bc1 is drawn with 1 <= |bc1| <= 2 so that this holds (both signs occur).  value_coef and entropy_coef
are float32 inputs (their fp32 values enter the fp64 formulas).

The bound is derived, never fitted (u = 2^-24, first order in u).  Rules: a sum of n products in ANY order plus a bias and a final
scaling is off by at most (n + 4) u sum |a| |b| (ppo_grad_ref's, with the bias); inherited errors propagate through the next
product; leaky(z) for z <= 0 costs 2 u |leaky(z)| (the fp32 slope and one product).
  h1     E_h1 = 2 u |h1| [z1 < 0];  x  E_x = E_h1 |W2|^T + (S + 4) u (|h1| |W2|^T + |b2|);  logits  E_l = E_x |Wd|^T + (S + 4) u |x| |Wd|^T
  xbar   E_xb = mean E_x + (N + 4) u mean |x|;  m  E_m = E_xb |Wc1|^T + (S + 4) u (|xbar| |Wc1|^T + |bc1|)
  a      E_a = leaky'(m) E_m + 2 u |a| [m < 0];  V  E_V = E_a . |Wc2| + (S + 4) u (|a| . |Wc2| + |bc2|)
  delta  E_delta = E_V + u |delta|;  delta^2: 2 |delta| E_delta + u delta^2
  d      E_d = E_l0 + E_l1 + u |d|.  The two-action softmax as a sigmoid of d (ppo_grad_ref): p_taken is off by rel_a = E_d p_other +
         8 u, p_other by rel_o = E_d p_taken + 8 u (exp within 3 ulp = 6 u, the sum, the quotient).
  NEW: log p.  spn(d) = max(-d, 0) + log1p(exp(-|d|)) is softplus(-d) for every d, so it inherits |d softplus(-d) / dd| E_d = p_other
         E_d; its own roundings: exp within 6 u t, passed on by log1p' = 1 / (1 + t) (6 u t / (1 + t) <= 6 u p_small), log1p within 2
         ulp = 4 u log1p(t), the final sum u spn.  E_spn = p_other E_d + u (6 p_small + 4 log1p(t) + spn);  E_spp the same with
         p_taken and spp.  action term delta spn: |delta| E_spn + spn E_delta + u |delta spn|.
  NEW: H.  H = p_taken spn + p_other spp, two products and a sum of positive terms:
         E_H = p_taken spn rel_a + p_taken E_spn + p_other spp rel_o + p_other E_spp + 2 u H.
  losses (sum E_term + (R + 2) u sum |term|) / R
  g      e2 = ec p_taken d: E_e2 = |ec| p_taken (|d| rel_a + E_d) + 2 u |e2|;  e3 = e2 - delta: E_e3 = E_e2 + E_delta + u |e3|;
         e4 = p_other e3: E_e4 = p_other E_e3 + |e4| (rel_o + u);  g = inv e4: E_g = inv E_e4 + 2 u |g|
  dV     E_dV = |cv| (sum_n E_delta + (N + 4) u sum_n |delta|);  da  E_da = leaky'(m) E_dV |Wc2| + 3 u |da|
  dxbar / N   E_q = (E_da |Wc1| + (S + 4) u |da| |Wc1|) / N;  dx  E_dx = E_g (|Wd_0| + |Wd_1|) + E_q + 4 u (|dl| |Wd| + |q|)
  dz1    E_dz1 = leaky'(z1) (E_dx |W2| + (S + 4) u |dx| |W2|) + 2 u |dz1|
  dW, db sum_r (E_dz |in| + |dz| E_in) + (rows + 2) u sum_r |dz| |in|      (in = in / h1 / xbar / a / x / 1 with their own errors)
  attention (tests/tarmac_ref.py's rule with the band replaced by all N senders, q, k, v inheriting E_x):
         E_q = E_x |Wq|^T + (S + 4) u (|x| |Wq|^T + |bq|), E_k, E_v alike;  E_s(i, j) = (sum_k (E_q |k| + |q| E_k) + (K + 4) u sum_k |q| |k|)
         / sqrt(C), E_s(i) = max_j;  every weight is off by rel = 2 E_s(i) + (N + 15) u + u max_j |s_ij - max_j s|  (the N - 1 other
         senders take c's place; the last term is the rounding of the subtracted maximum);  attn: attn rel;
         comm_out: sum_j attn (rel + (N + 4) u) |v| + attn E_v.
"""
import functools

import numpy as np

from tests.ppo_grad_ref import U, _grid, _mm, ratio_to_bound, worst  # noqa: F401

# (N, F, C, S, K)
SHAPES = [(1, 3, 4, 16, 4), (2, 5, 8, 20, 8), (5, 22, 8, 36, 16), (17, 7, 4, 64, 16), (20, 51, 32, 128, 16), (50, 51, 32, 128, 16),
          (64, 8, 32, 128, 16)]
STEPS = [1, 3, 16, 17, 33]
PARENT_STEPS = 33
SLOPE = 0.01
VALUE_COEF, ENTROPY_COEF = np.float32(0.5), np.float32(0.01)
PARAM_NAMES = ("W1", "b1", "W2", "b2", "Wc1", "bc1", "Wc2", "bc2", "Wq", "bq", "Wk", "bk", "Wv", "bv", "Wd")
REACHED = ("W1", "b1", "W2", "b2", "Wc1", "bc1", "Wc2", "bc2", "Wd")
VARIANTS = ("scale_sqrt_k", "no_self", "relu", "leaky0_is_1", "entropy_sign", "value_mean_B_only", "adv_not_detached", "per_agent_value",
            "dist_bias", "ret_not_gathered")
FLOAT_KEYS = ("logits", "value", "x", "comm_out", "attn", "losses", "advantage", "grad")


@functools.lru_cache(maxsize=None)
def draw(N, F, C, S, K, steps=PARENT_STEPS, seed=0):
    """The seeded inputs of `steps` stored env-steps for one shape, float32 / int64, read-only."""
    r = np.random.default_rng([seed, 0xA2C, N, F, C, S, K, steps])
    sign = r.integers(0, 2, S) * 2 - 1
    d = dict(obs=_grid(r, -4, 4, 4, (steps, N, F)), comm=_grid(r, -4, 4, 4, (steps, N, C)), ret=_grid(r, -12, 12, 4, (steps, N)),
             W1=_grid(r, -4, 4, 8, (S, F + C)), b1=_grid(r, -8, 8, 32, S), W2=_grid(r, -4, 4, 64, (S, S)), b2=_grid(r, -8, 8, 32, S),
             Wc1=_grid(r, -4, 4, 64, (S, S)), bc1=sign * _grid(r, 32, 64, 32, S), Wc2=_grid(r, -4, 4, 16, (1, S)), bc2=_grid(r, -8, 8, 32, 1),
             Wq=_grid(r, -4, 4, 8, (K, S)), bq=_grid(r, -8, 8, 32, K), Wk=_grid(r, -4, 4, 8, (K, S)), bk=_grid(r, -8, 8, 32, K),
             Wv=_grid(r, -4, 4, 16, (C, S)), bv=_grid(r, -8, 8, 32, C), Wd=_grid(r, -4, 4, 16, (2, S)))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d["action"] = r.integers(0, 2, (steps, N)).astype(np.int64)
    for v in d.values():
        v.setflags(write=False)
    return d


PER_STEP = ("obs", "comm", "ret", "action")


def inputs(B, N, F, C, S, K):
    """The first B env-steps of the shape's draw (a draw of its own beyond PARENT_STEPS)."""
    d = draw(N, F, C, S, K, steps=max(B, PARENT_STEPS))
    return {k: (v[:B] if k in PER_STEP else v) for k, v in d.items()}


def _rows(d, index):
    M = d["obs"].shape[0]
    return np.arange(M) if index is None else np.asarray(index, dtype=np.int64)


def _leaky(z, slope):
    return np.where(z > 0, z, slope * z).astype(z.dtype)


def _head(l, act, dt):
    """The two-action head on logits [R, 2]: dict(d, t, pa, po, spn, spp, H, small, lse) in dtype dt."""
    rows = np.arange(l.shape[0])
    dd = (l[rows, act] - l[rows, 1 - act]).astype(dt)
    t = np.exp(-np.abs(dd)).astype(dt)
    den = (dt(1) + t).astype(dt)
    big, small = (dt(1) / den).astype(dt), (t / den).astype(dt)
    lse = np.log1p(t).astype(dt)
    pa, po = np.where(dd >= 0, big, small), np.where(dd >= 0, small, big)
    spn, spp = (np.maximum(-dd, 0) + lse).astype(dt), (np.maximum(dd, 0) + lse).astype(dt)
    H = ((pa * spn).astype(dt) + (po * spp).astype(dt)).astype(dt)
    return dict(d=dd, t=t, pa=pa, po=po, spn=spn, spp=spp, H=H, small=small, lse=lse)


def evaluate(d, dtype=np.float64, perm=False, variant=None, index=None, vc=VALUE_COEF, ec=ENTROPY_COEF):
    """-> dict(logits [R, 2], x [R, S], value [B], advantage [B, N], losses [3], grad [flat, REACHED order], comm_out [B, N, C], attn
    [B, N, N], z1, m) evaluated in `dtype`; `perm` permutes every contraction; `variant`: one of the deliberately wrong forms of
    VARIANTS; `index`: the env-steps of the minibatch (None: all, in order)."""
    dt = dtype
    j = _rows(d, index)
    B, (_, N, F) = len(j), d["obs"].shape
    P = {k: np.asarray(d[k], dtype=dt) for k in PARAM_NAMES}
    S, C, K = P["W2"].shape[0], d["comm"].shape[2], P["Wq"].shape[0]
    R = B * N
    o = (lambda k, s=0: np.random.default_rng(k + s).permutation(k)) if perm else (lambda k, s=0: None)
    slope = dt(0) if variant == "relu" else dt(SLOPE)
    inp = np.concatenate([np.asarray(d["obs"], dtype=dt)[j].reshape(R, F), np.asarray(d["comm"], dtype=dt)[j].reshape(R, C)], axis=1)
    z1 = (_mm(inp, P["W1"].T, o(F + C)) + P["b1"]).astype(dt)
    h1 = _leaky(z1, slope)
    x = (_mm(h1, P["W2"].T, o(S)) + P["b2"]).astype(dt)
    logits = _mm(x, P["Wd"].T, o(S, 1)).astype(dt)
    if variant == "dist_bias":
        logits = (logits + np.asarray([0.25, -0.125], dtype=dt)).astype(dt)
    per_agent = variant == "per_agent_value"
    xr = x.reshape(B, N, S)
    on = o(N, 2)
    xbar = ((xr if on is None else xr[:, on]).sum(axis=1, dtype=dt) / dt(N)).astype(dt)
    xc = x if per_agent else xbar                                          # the critic's rows
    m = (_mm(xc, P["Wc1"].T, o(S, 3)) + P["bc1"]).astype(dt)
    a = _leaky(m, slope)
    Vc = (_mm(a, P["Wc2"].T, o(S, 4))[:, 0] + P["bc2"][0]).astype(dt)
    V = Vc.reshape(B, N).mean(axis=1).astype(dt) if per_agent else Vc
    Vr = Vc if per_agent else np.repeat(Vc, N)
    ret = np.asarray(d["ret"], dtype=dt)[np.arange(B) if variant == "ret_not_gathered" else j].reshape(R)
    act = np.asarray(d["action"])[j].reshape(R)
    delta = (ret - Vr).astype(dt)
    h = _head(logits, act, dt)
    cnt_v = B if variant == "value_mean_B_only" else R
    sq, al = (delta * delta).astype(dt), (delta * h["spn"]).astype(dt)
    losses = np.asarray([sq.sum(dtype=dt) / dt(cnt_v), al.sum(dtype=dt) / dt(R), h["H"].sum(dtype=dt) / dt(R)], dtype=dt)
    inv, vcf, ecf = dt(1.0 / R), dt(vc), dt(-ec if variant == "entropy_sign" else ec)
    e3 = ((ecf * h["pa"]).astype(dt) * h["d"]).astype(dt) - delta
    g = (inv * (h["po"] * e3.astype(dt)).astype(dt)).astype(dt)
    rows = np.arange(R)
    dl = np.zeros((R, 2), dtype=dt)
    dl[rows, act], dl[rows, 1 - act] = g, -g
    cv = dt(-2.0 * float(vcf) / cnt_v)
    dV = (cv * delta).astype(dt) if per_agent else (cv * (delta.reshape(B, N) if on is None else delta.reshape(B, N)[:, on]).sum(axis=1, dtype=dt)).astype(dt)
    if variant == "adv_not_detached":      # d action_loss / d V = sum log p / R
        lp = -h["spn"]
        dV = (dV + inv * (lp if per_agent else lp.reshape(B, N).sum(axis=1, dtype=dt))).astype(dt)
    mask_m = np.where((m >= 0) if variant == "leaky0_is_1" else (m > 0), dt(1), slope)
    da = ((dV[:, None] * P["Wc2"]).astype(dt) * mask_m).astype(dt)
    dxc = _mm(da, P["Wc1"], o(S, 5)).astype(dt)
    q = dxc if per_agent else np.repeat((dxc / dt(N)).astype(dt), N, axis=0)
    dx = (_mm(dl, P["Wd"], None) + q).astype(dt)
    mask1 = np.where((z1 >= 0) if variant == "leaky0_is_1" else (z1 > 0), dt(1), slope)
    dz1 = (_mm(dx, P["W2"], o(S, 6)) * mask1).astype(dt)
    oR, oc = o(R, 7), o(xc.shape[0], 8)
    one, onec = np.ones((R, 1), dtype=dt), np.ones((xc.shape[0], 1), dtype=dt)
    gl = [_mm(dz1.T, inp, oR), _mm(dz1.T, one, oR), _mm(dx.T, h1, oR), _mm(dx.T, one, oR), _mm(da.T, xc, oc), _mm(da.T, onec, oc),
          _mm(dV[None, :], a, oc), _mm(dV[None, :], onec, oc), _mm(dl.T, x, oR)]
    # the attention over the agents of every env-step
    qq = (_mm(x, P["Wq"].T, o(S, 9)) + P["bq"]).astype(dt).reshape(B, N, K)
    kk = (_mm(x, P["Wk"].T, o(S, 10)) + P["bk"]).astype(dt).reshape(B, N, K)
    vv = (_mm(x, P["Wv"].T, o(S, 11)) + P["bv"]).astype(dt).reshape(B, N, C)
    s = (np.einsum("bik,bjk->bij", qq, kk).astype(dt) / dt(np.sqrt(K if variant == "scale_sqrt_k" else C))).astype(dt)
    if variant == "no_self" and N > 1:
        s = np.where(np.eye(N, dtype=bool)[None], -np.inf, s).astype(dt)
    e = np.exp(s - s.max(axis=2, keepdims=True)).astype(dt)
    attn = (e / e.sum(axis=2, keepdims=True, dtype=dt)).astype(dt)
    comm_out = np.einsum("bij,bjc->bic", attn, vv).astype(dt)
    return dict(logits=logits, x=x, value=V, advantage=delta.reshape(B, N), losses=losses,
                grad=np.concatenate([t.astype(dt).reshape(-1) for t in gl]), comm_out=comm_out, attn=attn, z1=z1, m=m, dl=dl)


def bound(d, index=None, vc=VALUE_COEF, ec=ENTROPY_COEF):
    """-> dict(FLOAT_KEYS..., m): the module docstring's bounds, in fp64 on the exact quantities."""
    j = _rows(d, index)
    B, (_, N, F) = len(j), d["obs"].shape
    P = {k: np.asarray(d[k], dtype=np.float64) for k in PARAM_NAMES}
    A = {k: np.abs(v) for k, v in P.items()}
    S, C, K = P["W2"].shape[0], d["comm"].shape[2], P["Wq"].shape[0]
    R = B * N
    inp = np.concatenate([np.asarray(d["obs"], dtype=np.float64)[j].reshape(R, F), np.asarray(d["comm"], dtype=np.float64)[j].reshape(R, C)], axis=1)
    z1 = inp @ P["W1"].T + P["b1"]
    h1 = _leaky(z1, SLOPE)
    E_h1 = 2 * U * np.abs(h1) * (z1 < 0)
    x = h1 @ P["W2"].T + P["b2"]
    E_x = E_h1 @ A["W2"].T + (S + 4) * U * (np.abs(h1) @ A["W2"].T + A["b2"])
    logits = x @ P["Wd"].T
    E_l = E_x @ A["Wd"].T + (S + 4) * U * (np.abs(x) @ A["Wd"].T)
    xbar = x.reshape(B, N, S).mean(axis=1)
    E_xb = E_x.reshape(B, N, S).mean(axis=1) + (N + 4) * U * np.abs(x).reshape(B, N, S).mean(axis=1)
    m = xbar @ P["Wc1"].T + P["bc1"]
    E_m = E_xb @ A["Wc1"].T + (S + 4) * U * (np.abs(xbar) @ A["Wc1"].T + A["bc1"])
    a = _leaky(m, SLOPE)
    lm = np.where(m > 0, 1.0, SLOPE)
    E_a = lm * E_m + 2 * U * np.abs(a) * (m < 0)
    V = a @ P["Wc2"][0] + P["bc2"][0]
    E_V = E_a @ A["Wc2"][0] + (S + 4) * U * (np.abs(a) @ A["Wc2"][0] + A["bc2"][0])
    ret = np.asarray(d["ret"], dtype=np.float64)[j].reshape(R)
    act = np.asarray(d["action"])[j].reshape(R)
    delta = ret - np.repeat(V, N)
    E_delta = np.repeat(E_V, N) + U * np.abs(delta)
    h = _head(logits, act, np.float64)
    dd, pa, po, spn, spp, H = h["d"], h["pa"], h["po"], h["spn"], h["spp"], h["H"]
    E_d = E_l[:, 0] + E_l[:, 1] + U * np.abs(dd)
    rel_a, rel_o = E_d * po + 8 * U, E_d * pa + 8 * U
    own = 6 * h["small"] + 4 * h["lse"]
    E_spn, E_spp = po * E_d + U * (own + spn), pa * E_d + U * (own + spp)
    terms = np.stack([delta * delta, delta * spn, H])
    E_terms = np.stack([2 * np.abs(delta) * E_delta + U * delta * delta, np.abs(delta) * E_spn + spn * E_delta + U * np.abs(delta * spn),
                        pa * spn * rel_a + pa * E_spn + po * spp * rel_o + po * E_spp + 2 * U * H])
    E_losses = (E_terms.sum(axis=1) + (R + 2) * U * np.abs(terms).sum(axis=1)) / R
    inv, vcf, ecf = 1.0 / R, float(vc), float(ec)
    e2 = ecf * pa * dd
    E_e2 = abs(ecf) * pa * (np.abs(dd) * rel_a + E_d) + 2 * U * np.abs(e2)
    e3 = e2 - delta
    E_e3 = E_e2 + E_delta + U * np.abs(e3)
    e4 = po * e3
    E_e4 = po * E_e3 + np.abs(e4) * (rel_o + U)
    g = inv * e4
    E_g = inv * E_e4 + 2 * U * np.abs(g)
    rows = np.arange(R)
    dl = np.zeros((R, 2))
    dl[rows, act], dl[rows, 1 - act] = g, -g
    E_dl = np.repeat(E_g[:, None], 2, axis=1)
    cv = -2.0 * vcf / R
    dV = cv * delta.reshape(B, N).sum(axis=1)
    E_dV = abs(cv) * (E_delta.reshape(B, N).sum(axis=1) + (N + 4) * U * np.abs(delta).reshape(B, N).sum(axis=1))
    da = dV[:, None] * P["Wc2"] * lm
    E_da = lm * E_dV[:, None] * A["Wc2"] + 3 * U * np.abs(da)
    q = (da @ P["Wc1"]) / N
    E_q = (E_da @ A["Wc1"] + (S + 4) * U * (np.abs(da) @ A["Wc1"])) / N
    qr, E_qr = np.repeat(q, N, axis=0), np.repeat(E_q, N, axis=0)
    dx = dl @ P["Wd"] + qr
    E_dx = E_dl @ A["Wd"] + E_qr + 4 * U * (np.abs(dl) @ A["Wd"] + np.abs(qr))
    l1 = np.where(z1 > 0, 1.0, SLOPE)
    dz1 = (dx @ P["W2"]) * l1
    E_dz1 = l1 * (E_dx @ A["W2"] + (S + 4) * U * (np.abs(dx) @ A["W2"])) + 2 * U * np.abs(dz1)

    def acc(E_dz, dz, inn, E_in=None):
        n = dz.shape[0]
        e = E_dz.T @ np.abs(inn) + (n + 2) * U * (np.abs(dz).T @ np.abs(inn))
        if E_in is not None:
            e = e + np.abs(dz).T @ E_in
        return e.reshape(-1)

    one, oneb = np.ones((R, 1)), np.ones((B, 1))
    grad = np.concatenate([acc(E_dz1, dz1, inp), acc(E_dz1, dz1, one), acc(E_dx, dx, h1, E_h1), acc(E_dx, dx, one), acc(E_da, da, xbar, E_xb),
                           acc(E_da, da, oneb), acc(E_dV[:, None], dV[:, None], a, E_a), acc(E_dV[:, None], dV[:, None], oneb),
                           acc(E_dl, dl, x, E_x)])
    # the attention
    qq, kk, vv = (x @ P["W" + n].T + P["b" + n] for n in "qkv")
    E_qq, E_kk, E_vv = (E_x @ A["W" + n].T + (S + 4) * U * (np.abs(x) @ A["W" + n].T + A["b" + n]) for n in "qkv")
    qq, kk, E_qq, E_kk = (t.reshape(B, N, K) for t in (qq, kk, E_qq, E_kk))
    vv, E_vv = vv.reshape(B, N, C), E_vv.reshape(B, N, C)
    rc = np.sqrt(C)
    s = np.einsum("bik,bjk->bij", qq, kk) / rc
    E_sij = (np.einsum("bik,bjk->bij", E_qq, np.abs(kk)) + np.einsum("bik,bjk->bij", np.abs(qq), E_kk)
             + (K + 4) * U * np.einsum("bik,bjk->bij", np.abs(qq), np.abs(kk))) / rc
    mx = s.max(axis=2, keepdims=True)
    e = np.exp(s - mx)
    attn = e / e.sum(axis=2, keepdims=True)
    rel = 2 * E_sij.max(axis=2) + (N + 15) * U + U * np.abs(s - mx).max(axis=2)                # [B, N]
    E_comm = np.einsum("bij,bjc->bic", attn, np.abs(vv)) * (rel + (N + 4) * U)[:, :, None] + np.einsum("bij,bjc->bic", attn, E_vv)
    return dict(logits=E_l, x=E_x, value=E_V, advantage=E_delta.reshape(B, N), losses=E_losses, grad=grad, comm_out=E_comm,
                attn=attn * rel[:, :, None], m=E_m)


def admitted(ref, bnd):
    """Is the critic's LeakyReLU mask of this case beyond rounding?  Every |m| in fp64 above 8 times its own bound."""
    return bool((np.abs(ref["m"]) > 8 * bnd["m"]).all())


def z1_is_exact(d, index=None):
    """z1 in fp32 under a permuted summation equals the fp64 value bit for bit."""
    a, b = evaluate(d, np.float32, perm=True, index=index)["z1"], evaluate(d, np.float64, index=index)["z1"]
    return bool(np.array_equal(a.astype(np.float64), b))


def param_slices(F, C, S):
    sizes = [S * (F + C), S, S * S, S, S * S, S, S, 1, 2 * S]
    off = np.concatenate([[0], np.cumsum(sizes)])
    return {n: slice(int(off[i]), int(off[i + 1])) for i, n in enumerate(REACHED)}


def worst_of(got, ref, bnd, keys=FLOAT_KEYS):
    """The largest |error| / bound over the float outputs named."""
    return max(worst(got[k], ref[k], bnd[k]) for k in keys if k in got)


@functools.lru_cache(maxsize=None)
def reference(B, N, F, C, S, K):
    """The inputs, the fp64 values and the bounds of one case, computed once and shared read-only: dict(inputs, ref, bound)."""
    d = inputs(B, N, F, C, S, K)
    ref, bnd = evaluate(d), bound(d)
    for t in list(ref.values()) + list(bnd.values()):
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return dict(inputs=d, ref=ref, bound=bnd)


# ---- the recorded reference cases (tests/golden/tarmac_a2c_cases.npz, written by tests/golden/make_tarmac_a2c_golden.py)

SD_KEYS = dict(W1="base.common.0.weight", b1="base.common.0.bias", W2="base.common.2.weight", b2="base.common.2.bias",
               Wc1="base.critic.0.weight", bc1="base.critic.0.bias", Wc2="base.critic.3.weight", bc2="base.critic.3.bias",
               Wq="base.comm.state2query.weight", bq="base.comm.state2query.bias", Wk="base.comm.state2key.weight",
               bk="base.comm.state2key.bias", Wv="base.comm.state2value.weight", bv="base.comm.state2value.bias", Wd="dist.linear.weight")


@functools.lru_cache(maxsize=None)
def load_cases():
    """name -> dict(N, F, C, S, K, B, vc, ec, sd {key: float32}, inputs (the dict `evaluate` takes), value, logits, x, comm_out, p_attn,
    losses (float64), grad {key: float64}, no_grad [names])."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tarmac_a2c_cases.npz")
    cases = {}
    with np.load(path) as z:
        for name in z["names"]:
            name = str(name)
            N, F, C, S, K, B = (int(x) for x in z[name + "/meta"])
            sd = {k[len(name) + 4:]: z[k] for k in z.files if k.startswith(name + "/sd/")}
            grad = {k[len(name) + 6:]: z[k] for k in z.files if k.startswith(name + "/grad/")}
            d = dict({p: sd[key] for p, key in SD_KEYS.items()}, obs=z[name + "/obs"], comm=z[name + "/comm_in"], ret=z[name + "/returns"],
                     action=z[name + "/action"])
            c = dict(N=N, F=F, C=C, S=S, K=K, B=B, vc=float(z[name + "/coef"][0]), ec=float(z[name + "/coef"][1]), sd=sd, inputs=d, grad=grad,
                     no_grad=[str(s) for s in z[name + "/no_grad"]])
            for k in ("value", "logits", "x", "comm_out", "p_attn", "losses"):
                c[k] = z[name + "/" + k]
            cases[name] = c
    return cases


def golden_flat_grad(case):
    """The recorded gradients of the nine reached tensors as one flat float64 vector in REACHED order."""
    return np.concatenate([case["grad"][SD_KEYS[p]].reshape(-1) for p in REACHED])


def make_policy(case):
    """A TarMACA2CPolicy (CPU, float32) holding a recorded case's weights, loaded strictly."""
    import torch
    from mdr_amd.tarmac_a2c import TarMACA2CPolicy
    policy = TarMACA2CPolicy(case["F"], state_size=case["S"], comm_size=case["C"], key_size=case["K"])
    policy.load_state_dict({k: torch.from_numpy(np.array(w)) for k, w in case["sd"].items()}, strict=True)
    return policy
