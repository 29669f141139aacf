"""A plain fp64 restatement of the TarMAC-PPO actor (agents/network.py:103-238) and of what mdr_tarmac_comm / mdr_logits_sample
compute (include/mdr_policy.h): the sender offsets of make_masks, the banded attention, the dense masked attention it restates, the
whole actor forward on a state_dict, the Philox dead-sender draws, and a running rounding-error bound for the attention.  numpy on
the CPU only; tests/test_tarmac.py and tests/test_gpu_tarmac.py hold the product to it.

The bound is derived, never fitted to what a kernel returns (u = 2^-24, K = num_key, V = num_value, c + 1 senders per receiver):

  scores   score_s = (sum_k q_k key_sk) / sqrt(K) as a chain of K fp32 fmas and one multiplication by the rounded 1 / sqrt(K): off
           by at most gamma_K plus two roundings (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), i.e.
           E_s = (K + 2) u max_s sum_k |q_k| |key_sk| / sqrt(K), taken over the receiver's live senders.
  weights  exp(score_s - max) sees both scores off by E_s: 2 E_s relative.  The exponential itself is allowed a few ulp plus the
           |score_s - max| u of a fast exp (argument times log2 e, rounded, into exp2) - a term that only matters where the weight
           is exp(-|score_s - max|) small; the (c + 1)-term sum of the weights adds c u, the reciprocal and its product two more:
           (c + 16) u covers them, hence 2 E_s + (c + 16) u relative on every attention weight.
  values   comm = sum_s attn_s value_s as a (c + 1)-term fma chain, at most (c + 1) u of sum attn |value| more; the issue's
           budget writes c + V + 16 for the sum of the last two, which is what is used:
           bound_comm = (2 E_s + (c + V + 16) u) sum_s attn_s |value_s|.
"""
import numpy as np

from oracle.mdr_oracle import philox4x32_10
from tests.actor_ref import uniform_of

TAG_TARMAC = 0x544D4331
U_FP32 = 2.0 ** -24
NEIGHBOURS, NONE = 0, 1      # mdr_tarmac_mode


def offsets(nb_comm, swapped=False):
    """Sender offsets after the receiver itself: offset number i >= 1 is +(i + 1) / 2 for odd i and -i / 2 for even i.
    `swapped`: the deliberately wrong variant with the signs exchanged."""
    out = [(i + 1) // 2 if i % 2 else -(i // 2) for i in range(1, int(nb_comm) + 1)]
    return [-o for o in out] if swapped else out


def clamp(nb_comm, nb_agents):
    return min(int(nb_comm), int(nb_agents) - 1)


def sender_index(nb_agents, nb_comm, swapped=False):
    """int [N, c + 1]: column 0 the receiver itself, then its c senders."""
    N = int(nb_agents)
    off = np.array([0] + offsets(clamp(nb_comm, N), swapped), dtype=np.int64)
    return (np.arange(N)[:, None] + off[None, :]) % N


def band_mask(nb_agents, nb_comm, mode=NEIGHBOURS):
    """bool [receiver, sender]; mode none: all zero, no diagonal."""
    N = int(nb_agents)
    mask = np.zeros((N, N), dtype=bool)
    if mode == NONE:
        return mask
    idx = sender_index(N, nb_comm)
    mask[np.arange(N)[:, None], idx] = True
    return mask


def band_attention(q, k, v, nb_comm, mode=NEIGHBOURS, dead=None, dtype=np.float64, swapped=False, scale=True, with_self=True):
    """q, k [E, N, K], v [E, N, V] -> (comm [E, N, V], bound_comm [E, N, V]) evaluated in `dtype`.  `dead` bool [E, N]: silenced
    senders (a receiver always hears itself).  `swapped` / `scale=False` / `with_self=False`: the three wrong variants
    tests/test_tarmac.py uses to show that the bound discriminates."""
    q, k, v = (np.asarray(t, dtype=dtype) for t in (q, k, v))
    E, N, K = q.shape
    V = v.shape[2]
    if mode == NONE:
        return np.zeros((E, N, V), dtype=dtype), np.zeros((E, N, V))
    c = clamp(nb_comm, N)
    idx = sender_index(N, nb_comm, swapped)                              # [N, c + 1]
    ks, vs = k[:, idx], v[:, idx]                                        # [E, N, c + 1, K | V]
    alive = np.ones((E, N, c + 1), dtype=bool)
    if dead is not None:
        alive = ~np.asarray(dead, dtype=bool)[:, idx]
        alive[:, :, 0] = True
    if not with_self:
        alive = alive.copy()
        alive[:, :, 0] = False
    inv = dtype(1.0 / np.sqrt(dtype(K))) if scale else dtype(1.0)
    s = np.einsum("enk,enck->enc", q, ks).astype(dtype) * inv
    s = np.where(alive, s, -np.inf)
    m = s.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(alive, np.exp(s - m), 0).astype(dtype)
    attn = e / e.sum(axis=2, keepdims=True, dtype=dtype)
    attn = np.where(np.isnan(attn), 0, attn).astype(dtype)
    comm = np.einsum("enc,encv->env", attn, vs).astype(dtype)
    mag = np.einsum("enk,enck->enc", np.abs(q).astype(np.float64), np.abs(ks).astype(np.float64)) / np.sqrt(K)
    e_s = (K + 2) * U_FP32 * np.where(alive, mag, 0).max(axis=2)         # [E, N]
    bound = (2 * e_s + (c + V + 16) * U_FP32)[:, :, None] * np.einsum("enc,encv->env", attn.astype(np.float64), np.abs(vs).astype(np.float64))
    return comm, bound


def dense_attention(q, k, v, nb_comm, mode=NEIGHBOURS, dead=None):
    """TarMAC_Comm.forward's dense form in fp64: the full score matrix, the maximum of the UNMASKED row subtracted, exp times mask,
    normalised, NaN -> 0."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    E, N, K = q.shape
    mask = np.broadcast_to(band_mask(N, nb_comm, mode)[None], (E, N, N))
    if dead is not None and mode == NEIGHBOURS:
        mask = mask & ~np.asarray(dead, dtype=bool)[:, None, :]
        mask = mask | np.eye(N, dtype=bool)[None]
    s = q @ k.transpose(0, 2, 1) / np.sqrt(K)
    s = s - s.max(axis=2, keepdims=True)
    e = np.exp(s) * mask
    with np.errstate(invalid="ignore", divide="ignore"):
        attn = e / e.sum(axis=2, keepdims=True)
    attn = np.where(np.isnan(attn), 0.0, attn)
    return attn @ v


def _mlp(sd, prefix, x, act):
    h = x @ sd[prefix + ".0.weight"].T + sd[prefix + ".0.bias"]
    h = np.maximum(h, 0.0) if act == "relu" else np.tanh(h)
    return h @ sd[prefix + ".2.weight"].T + sd[prefix + ".2.bias"]


def actor_forward(sd, obs, nb_comm, num_hops=1, mode=NEIGHBOURS, with_comm=True, dead=None, dense=False):
    """TarMAC_Actor.forward in fp64 on a state_dict of numpy arrays: obs [E, N, F] -> probabilities [E, N, 2].  `dead`: per hop, a
    list of bool [E, N] (or None).  `dense`: through dense_attention instead of band_attention."""
    sd = {n: np.asarray(w, dtype=np.float64) for n, w in sd.items()}
    x = _mlp(sd, "obs2hidden", np.asarray(obs, dtype=np.float64), "relu")
    if not with_comm:
        logits = _mlp(sd, "hidden2action", x, "relu")
    else:
        h, comm = x, None
        for hop in range(num_hops):
            if hop > 0:
                h = _mlp(sd, "comm.msg_state2state", np.concatenate([comm, h], axis=2), "tanh")      # comm first
            key, value, query = (_mlp(sd, "comm.hidden2" + n, h, "tanh") for n in ("key", "value", "query"))
            d = dead[hop] if dead is not None else None
            comm = dense_attention(query, key, value, nb_comm, mode, d) if dense else band_attention(query, key, value, nb_comm, mode, d)[0]
        logits = _mlp(sd, "comm_hidden2action", np.concatenate([x, comm], axis=2), "relu")          # the ORIGINAL hidden state
    z = logits - logits.max(axis=2, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=2, keepdims=True)


def dead_uniform(nb_envs, nb_agents, seed, step, step_dev=0, hop=0):
    """The float32 uniform behind every sender's defect draw, [E, N]: word `hop` of Philox4x32-10 with key = (seed lo, seed hi) and
    counter = (agent lo, agent hi, (step lo + step_dev) mod 2^32, TAG_TARMAC ^ step hi), agent = env * N + house, through
    actor_ref.uniform_of."""
    agent = np.arange(int(nb_envs) * int(nb_agents), dtype=np.uint64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    c2 = ((step & 0xFFFFFFFF) + (int(step_dev) & 0xFFFFFFFF)) & 0xFFFFFFFF
    words = philox4x32_10(agent & np.uint64(0xFFFFFFFF), agent >> np.uint64(32), c2, TAG_TARMAC ^ (step >> 32), seed & 0xFFFFFFFF, seed >> 32)
    return uniform_of(words[hop].astype(np.uint32)).reshape(int(nb_envs), int(nb_agents))


def dead_mask(nb_envs, nb_agents, prob, seed, step, step_dev=0, hop=0):
    """bool [E, N]: sender dead iff u < prob, compared in float32; prob == 0 draws nothing."""
    if prob <= 0:
        return np.zeros((int(nb_envs), int(nb_agents)), dtype=bool)
    return dead_uniform(nb_envs, nb_agents, seed, step, step_dev, hop) < np.float32(prob)


# ---- the inputs of tests/test_gpu_tarmac.py, built on the CPU so that tests/test_tarmac.py can judge them without a kernel

# (E, N, c, K, V): the smallest shapes that reach each tiling and band corner of k_tarmac_comm
COMM_CASES = [
    (3, 1, 10, 8, 16),        # self only
    (4, 2, 10, 8, 16),        # the clamp
    (5, 5, 4, 8, 16),         # every other agent, full wrap
    (5, 6, 3, 8, 16),         # odd, asymmetric band
    (7, 11, 10, 8, 16),
    (13, 20, 10, 8, 16),      # 12 envs per tile plus a tile holding one env
    (6, 50, 10, 8, 16),
    (2, 256, 10, 8, 16),      # exactly one tile per env
    (2, 300, 10, 8, 16),      # slice + partial slice, halos that wrap and cross the slice boundary
    (1, 1024, 10, 8, 16),
    (2, 64, 63, 8, 16),       # the widest band
    (3, 20, 10, 4, 4),
    (2, 50, 7, 16, 32),
    (3, 20, 0, 8, 16),        # out == v bit for bit
    (2, 300, 10, 32, 64),     # the widest rows: the K <= 32, V <= 64 form on more than 64 KB of LDS
]
DEFECT_CASES = [(13, 20, 10, 8, 16), (2, 300, 10, 8, 16)]


def comm_inputs(E, N, K, V, seed=0):
    """N(0, 1) float32 query, key [E, N, K] and value [E, N, V]."""
    rng = np.random.default_rng([seed, E, N, K, V])
    return tuple(rng.standard_normal((E, N, d)).astype(np.float32) for d in (K, K, V))


# ---- the recorded reference cases (tests/golden/tarmac_actor_cases.npz, written by tests/golden/make_tarmac_golden.py)

def load_cases():
    """name -> dict(F, N, c, hops, mode, with_comm, H, K, V, obs float32 [4, N, F], probs float64 [4, N, 2], sd {key: float32 array})."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tarmac_actor_cases.npz")
    cases = {}
    with np.load(path) as z:
        for name in z["names"]:
            name = str(name)
            F, N, c, hops, mode, with_comm, H, K, V = (int(x) for x in z[name + "/meta"])
            prefix = name + "/sd/"
            cases[name] = dict(F=F, N=N, c=c, hops=hops, mode=mode, with_comm=bool(with_comm), H=H, K=K, V=V, obs=z[name + "/obs"],
                               probs=z[name + "/probs"], sd={k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)})
    return cases


def make_actor(case, attention="dense", defect_prob=0.0):
    """A TarMACActor (CPU, float32) holding a recorded case's weights, loaded strictly."""
    import torch
    from mdr_amd.tarmac import TarMACActor
    actor = TarMACActor(case["F"], num_key=case["K"], num_value=case["V"], hidden_state_size=case["H"], number_agents_comm=case["c"],
                        comm_mode="none" if case["mode"] == NONE else "neighbours", comm_defect_prob=defect_prob, num_hops=case["hops"],
                        with_comm=case["with_comm"], attention=attention)
    actor.load_state_dict({k: torch.from_numpy(np.array(w)) for k, w in case["sd"].items()}, strict=True)
    return actor
