"""The gradient of the banded TarMAC attention (mdr_tarmac_comm_backward, include/mdr_policy.h) restated in numpy on the CPU: the five
formulas of the two-pass evaluation in a chosen dtype, the dense fp64 gradient they must equal, and a per-element rounding bound.
tests/test_tarmac_grad.py holds the restatement and the bound to account, tests/test_gpu_tarmac_grad.py holds the kernels to them.
The forward's restatement, its sender offsets, its Philox draws and its inputs are those of tests/tarmac_ref.py.

Receiver r has the live senders S(r): itself and r + o (mod N) for the first c = min(nb_comm, N - 1) offsets +1, -1, +2, -2, ..., less
the senders other than r that the hop's draw silenced.  p_rs the masked softmax weight, out_r = sum_s p_rs v_s, g_r = dL / dout_r:

    delta_r = g_r . out_r                      ds_rs = p_rs (g_r . v_s - delta_r)
    dq_r = (1 / sqrt K) sum_{s in S(r)} ds_rs k_s
    dk_s = (1 / sqrt K) sum_{r: s in S(r)} ds_rs q_r        dv_s = sum_{r: s in S(r)} p_rs g_r          (s is heard by r = s - o)

The bound is derived, never fitted to what a kernel returns (u = 2^-24, K = num_key, V = num_value, c + 1 senders per receiver; first
order in u, every constant rounded up; hats are computed values):

  weights  tarmac_ref's: every p_rs is off by at most eps_r p_rs, eps_r = 2 E_r + (c + 16) u, E_r = (K + 2) u max_s sum_k |q_rk| |k_sk|
           / sqrt K over S(r) - two scores off by E_r each, the exponential, the (c + 1)-term sum, the reciprocal and its product.
           Recomputing p_rs in the sender-major pass from the stored maximum and 1 / sum is the same computation.
  g . v    a V-term fma chain: off by at most V u G_rs, G_rs = sum_j |g_rj| |v_sj|.
  delta    g_r . out_r is taken of the FORWARD's float32 out, which is itself off by tarmac_ref's bound_comm_rj = (2 E_r + (c + V + 16) u)
           sum_s p_rs |v_sj|; with the chain's own V u sum_j |g_rj| |out_rj|:
           D_r = V u sum_j |g_rj| |out_rj| + (2 E_r + (c + V + 16) u) sum_s p_rs G_rs.
  ds       t_rs = g . v - delta cancels; its ERROR does not shrink with it: |t^ - t| <= V u G_rs + D_r + u |t_rs| (the subtraction),
           i.e. the cancellation is paid through |g| . |v| and |g| . |out|, not through |t|.  The product with p^ adds eps_r and one
           rounding, the final scaling of the row one more:
           e_rs = p_rs ((eps_r + 3 u) |t_rs| + V u G_rs + D_r).
  dq, dk   (1 / sqrt K) sum ds x as a chain of at most c + 1 fmas, the rounded 1 / sqrt K, the multiplication by it and (receiver
           pass) by 1 / sum: (c + 4) u of sum |ds| |x| on top of the inherited sum e |x|:
           bound_dq_rj = (sum_s e_rs |k_sj| + (c + 4) u sum_s |ds_rs| |k_sj|) / sqrt K,    dk likewise over the receivers of s with |q_rj|.
  dv       sum_r p_rs g_rj: bound_dv_sj = sum_r (eps_r + (c + 2) u) p_rs |g_rj|.
"""
import functools

import numpy as np

from tests import tarmac_ref as tr

U = tr.U_FP32

# (E, N, c, K, V): the smallest shapes that reach each tiling and band corner of the two backward kernels
GRAD_CASES = [
    (3, 1, 10, 8, 16),        # self only
    (4, 2, 10, 8, 16),        # the clamp
    (5, 5, 4, 8, 16),         # every other agent
    (5, 6, 3, 8, 16),         # odd band: the mirror
    (13, 20, 10, 8, 16),      # several envs per tile plus a tile holding one
    (2, 256, 10, 8, 16),      # exactly one tile per env
    (2, 300, 10, 8, 16),      # slice plus partial slice, wrapped halos on both sides
    (2, 64, 63, 8, 16),       # the widest band
    (3, 20, 0, 8, 16),        # c = 0
    (3, 20, 10, 4, 4),        # the narrowest rows
    (2, 50, 7, 16, 32),       # wider rows
    (2, 300, 10, 32, 64),     # the widest rows, the LDS limit
]
DEFECT_CASES = [(13, 20, 10, 8, 16), (2, 300, 10, 8, 16)]
DEFECT_PROB, DEFECT_SEED, DEFECT_STEP_DEV = 0.3, 0x1234567890ABCDEF, 7
# (step, whether a step_dev tensor holding DEFECT_STEP_DEV is passed): the second wraps the low word
DEFECT_KEYS = [(5, False), ((3 << 32) + 0xFFFFFFFE, True)]


def grad_out(E, N, V, seed=0):
    """The seeded N(0, 1) float32 gradient of the loss with respect to the attention's output, [E, N, V]."""
    return np.random.default_rng([seed, 0x67, E, N, V]).standard_normal((E, N, V)).astype(np.float32)


def receiver_index(nb_agents, nb_comm, mirrored=True):
    """int [N, c + 1]: column i the receiver that hears sender s at offset number i (column 0: s itself), r = s - o.
    `mirrored=False`: the deliberately wrong r = s + o."""
    N = int(nb_agents)
    off = np.array([0] + tr.offsets(tr.clamp(nb_comm, N)), dtype=np.int64)
    return (np.arange(N)[:, None] + (-off if mirrored else off)[None, :]) % N


def band_grad(q, k, v, g, nb_comm, mode=tr.NEIGHBOURS, dead=None, dtype=np.float64, mirrored=True, use_delta=True, scale=True,
              sender_defects=True):
    """-> (dq, dk [E, N, K], dv [E, N, V]) evaluated in `dtype`, in the two passes the kernels take.  `dead` bool [E, N].  The four
    flags switch the wrong variants of tests/test_tarmac_grad.py on: receivers r = s + o, delta dropped, the 1 / sqrt K of dq and
    dk dropped, defects ignored in the sender-major pass."""
    q, k, v, g = (np.asarray(t, dtype=dtype) for t in (q, k, v, g))
    E, N, K = q.shape
    if mode == tr.NONE:
        return np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    c = tr.clamp(nb_comm, N)
    inv = dtype(1.0 / np.sqrt(dtype(K)))
    post = inv if scale else dtype(1.0)
    dead = np.zeros((E, N), dtype=bool) if dead is None else np.asarray(dead, dtype=bool)
    # ---- receiver-major: the statistics, delta and dq
    idx = tr.sender_index(N, nb_comm)                                    # [N, c + 1]
    ks, vs = k[:, idx], v[:, idx]
    alive = ~dead[:, idx]
    alive[:, :, 0] = True
    s = np.where(alive, np.einsum("enk,enck->enc", q, ks).astype(dtype) * inv, -np.inf)
    m = s.max(axis=2)
    e = np.where(alive, np.exp(s - m[:, :, None]), 0).astype(dtype)
    linv = (dtype(1.0) / e.sum(axis=2, dtype=dtype)).astype(dtype)
    p = e * linv[:, :, None]
    out = np.einsum("enc,encv->env", p, vs).astype(dtype)
    delta = np.einsum("env,env->en", g, out).astype(dtype) if use_delta else np.zeros((E, N), dtype=dtype)
    ds = p * (np.einsum("env,encv->enc", g, vs).astype(dtype) - delta[:, :, None])
    dq = (np.einsum("enc,enck->enk", ds, ks) * post).astype(dtype)
    # ---- sender-major: every sender recomputes the weight each of its receivers gives it from (m, 1 / l, delta) of that receiver
    ridx = receiver_index(N, nb_comm, mirrored)                          # [N, c + 1]
    qr, gr = q[:, ridx], g[:, ridx]
    heard = np.ones((E, N, c + 1), dtype=bool)
    if sender_defects:
        heard[:, :, 1:] = ~dead[:, :, None]
    sc = np.einsum("enck,enk->enc", qr, k).astype(dtype) * inv
    with np.errstate(over="ignore"):
        ps = np.where(heard, np.exp(sc - m[:, ridx]) * linv[:, ridx], 0).astype(dtype)
    dss = ps * (np.einsum("encv,env->enc", gr, v).astype(dtype) - delta[:, ridx])
    dk = (np.einsum("enc,enck->enk", dss, qr) * post).astype(dtype)
    dv = np.einsum("enc,encv->env", ps, gr).astype(dtype)
    return dq, dk, dv


def dense_mask(E, N, nb_comm, dead=None):
    mask = np.broadcast_to(tr.band_mask(N, nb_comm)[None], (E, N, N))
    if dead is not None:
        mask = (mask & ~np.asarray(dead, dtype=bool)[:, None, :]) | np.eye(N, dtype=bool)[None]
    return mask


def dense_grad(q, k, v, g, nb_comm, mode=tr.NEIGHBOURS, dead=None):
    """The closed-form fp64 gradient of the DENSE formula (tarmac_ref.dense_attention: the agents x agents scores under the mask):
    P = masked softmax, dP = g v^T, dS = P (dP - rowsum(P dP)), dq = dS k / sqrt K, dk = dS^T q / sqrt K, dv = P^T g.  No band
    arithmetic: the mirror of the sender-major pass is the transpose here."""
    q, k, v, g = (np.asarray(t, dtype=np.float64) for t in (q, k, v, g))
    E, N, K = q.shape
    if mode == tr.NONE:
        return np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    mask = dense_mask(E, N, nb_comm, dead)
    s = np.where(mask, q @ k.transpose(0, 2, 1) / np.sqrt(K), -np.inf)
    e = np.exp(s - s.max(axis=2, keepdims=True))
    P = e / e.sum(axis=2, keepdims=True)
    dP = g @ v.transpose(0, 2, 1)
    dS = P * (dP - (P * dP).sum(axis=2, keepdims=True))
    return dS @ k / np.sqrt(K), dS.transpose(0, 2, 1) @ q / np.sqrt(K), P.transpose(0, 2, 1) @ g


def _to_senders(idx, x):
    """x [E, N(receiver), c + 1, D] -> [E, N(sender), D]: every (receiver, slot) term added to the sender idx[receiver, slot]."""
    out = np.zeros((x.shape[0], x.shape[1], x.shape[3]))
    np.add.at(out, (slice(None), idx), x)
    return out


def grad_bound(q, k, v, g, nb_comm, mode=tr.NEIGHBOURS, dead=None):
    """-> (bound_dq, bound_dk [E, N, K], bound_dv [E, N, V]) of the module docstring, in fp64 on the exact quantities."""
    q, k, v, g = (np.asarray(t, dtype=np.float64) for t in (q, k, v, g))
    E, N, K = q.shape
    V = v.shape[2]
    if mode == tr.NONE:
        return np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    c = tr.clamp(nb_comm, N)
    idx = tr.sender_index(N, nb_comm)
    ks, vs = k[:, idx], v[:, idx]
    alive = np.ones((E, N, c + 1), dtype=bool)
    if dead is not None:
        alive = ~np.asarray(dead, dtype=bool)[:, idx]
        alive[:, :, 0] = True
    inv = 1.0 / np.sqrt(K)
    s = np.where(alive, np.einsum("enk,enck->enc", q, ks) * inv, -np.inf)
    e = np.exp(s - s.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    out = np.einsum("enc,encv->env", p, vs)
    delta = np.einsum("env,env->en", g, out)
    t = np.einsum("env,encv->enc", g, vs) - delta[:, :, None]
    ds = p * t
    mag = np.einsum("enk,enck->enc", np.abs(q), np.abs(ks)) * inv
    e_r = (K + 2) * U * np.where(alive, mag, 0).max(axis=2)               # [E, N]
    eps = 2 * e_r + (c + 16) * U
    G = np.einsum("env,encv->enc", np.abs(g), np.abs(vs))
    D = V * U * np.einsum("env,env->en", np.abs(g), np.abs(out)) + (2 * e_r + (c + V + 16) * U) * (p * G).sum(axis=2)
    e_ds = p * ((eps + 3 * U)[:, :, None] * np.abs(t) + V * U * G + D[:, :, None])
    chain = (c + 4) * U
    bq = inv * (np.einsum("enc,enck->enk", e_ds, np.abs(ks)) + chain * np.einsum("enc,enck->enk", np.abs(ds), np.abs(ks)))
    aq, ag = np.abs(q)[:, :, None, :], np.abs(g)[:, :, None, :]
    bk = inv * _to_senders(idx, (e_ds + chain * np.abs(ds))[:, :, :, None] * aq)
    bv = _to_senders(idx, ((eps + (c + 2) * U)[:, :, None] * p)[:, :, :, None] * ag)
    return bq, bk, bv


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0)."""
    return float(ratio(got, ref, bound).max())


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def defect_mask(shape, hop, key):
    E, N = shape[:2]
    step, with_dev = key
    return tr.dead_mask(E, N, DEFECT_PROB, DEFECT_SEED, step, DEFECT_STEP_DEV if with_dev else 0, hop)


@functools.lru_cache(maxsize=None)
def reference(shape, hop=None, key=None):
    """The inputs, the dead senders, the fp64 gradient and the bound of one case, computed once and shared read-only:
    dict(q, k, v, g float32; dead bool [E, N] or None; grad = (dq, dk, dv) fp64; bound = (bq, bk, bv)).  `hop`, `key` (an entry of
    DEFECT_KEYS): the defect cases."""
    E, N, c, K, V = shape
    q, k, v = tr.comm_inputs(E, N, K, V)
    g = grad_out(E, N, V)
    dead = defect_mask(shape, hop, key) if key is not None else None
    ref = dict(q=q, k=k, v=v, g=g, dead=dead, grad=dense_grad(q, k, v, g, c, dead=dead), bound=grad_bound(q, k, v, g, c, dead=dead))
    for x in (q, k, v, g) + ref["grad"] + ref["bound"] + ((dead,) if dead is not None else ()):
        x.setflags(write=False)
    return ref
