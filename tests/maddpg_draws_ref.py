"""numpy restatement of the device-side draws of one MADDPG update (include/mdr_policy.h: mdr_maddpg_draws), built on the oracle's
Philox4x32-10 and tests/minibatch_ref.half_width: the positions the kernel must give, one for one, and the gumbel noise in float64
cast to float32.  ``rounds`` and ``half_bits`` exist so that a test can build a deliberately wrong variant."""
import numpy as np

from oracle.mdr_oracle import philox4x32_10
from tests.minibatch_ref import M32, half_width

TAG_INDEX = 0x4D444931      # "MDI1"
TAG_NOISE = 0x4D444E31      # "MDN1"
MAX_AGENTS = 426            # MDR_MADDPG_DRAWS_MAX_AGENTS: 1280 joint inputs / (1 feature + 2)


def _counter(step, cursor, tag):
    """(c2, c3): step lo + cursor mod 2^32 with no carry, tag ^ step hi."""
    step = int(step) & 0xFFFFFFFFFFFFFFFF
    return ((step & M32) + (int(cursor) & M32)) & M32, tag ^ (step >> 32)


def _key(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def index(N, B, length, seed, step, cursor=0, rounds=4, half_bits=None):
    """int64 [N, B]: row a = the first B elements of agent a's Feistel permutation of ``length`` elements (cycle walking), the round
    function word .x of Philox on (R, (a << 8) | r, c2, TAG_INDEX ^ step hi).  ``length`` < 1 is read as 1, as the kernel reads a
    device length; B <= length is the caller's business."""
    length = max(int(length), 1)
    h = half_width(length) if half_bits is None else int(half_bits)
    mask = np.uint64((1 << h) - 1)
    c2, c3 = _counter(step, cursor, TAG_INDEX)
    k0, k1 = _key(seed)
    out = np.zeros((int(N), int(B)), dtype=np.int64)
    for a in range(int(N)):
        x = np.arange(int(B), dtype=np.uint64)
        todo = np.arange(int(B))
        while todo.size:
            L, R = x >> np.uint64(h), x & mask
            for r in range(rounds):
                f = philox4x32_10(R, (a << 8) | r, c2, c3, k0, k1)[0] & mask
                L, R = R, L ^ f
            x = (L << np.uint64(h)) | R
            done = x < np.uint64(length)
            out[a, todo[done]] = x[done].astype(np.int64)
            todo, x = todo[~done], x[~done]
    return out


def noise_words(N, B, seed, step, cursor=0):
    """uint32 [N, B, N + 1, 2]: words .x, .y of Philox on (q lo, q hi, c2, TAG_NOISE ^ step hi), q = (a B + b) (N + 1) + k."""
    c2, c3 = _counter(step, cursor, TAG_NOISE)
    k0, k1 = _key(seed)
    q = np.arange(int(N) * int(B) * (int(N) + 1), dtype=np.uint64)
    w = philox4x32_10(q & np.uint64(M32), q >> np.uint64(32), c2, c3, k0, k1)
    return np.stack([np.asarray(w[0], dtype=np.uint64), np.asarray(w[1], dtype=np.uint64)], -1).astype(np.uint32).reshape(int(N), int(B), int(N) + 1, 2)


def gumbel(words):
    """-log(-log((word + 0.5) / 2^32)) in float64 (the caller casts)."""
    u = (np.asarray(words, dtype=np.float64) + 0.5) / 4294967296.0
    return -np.log(-np.log(u))


def noise(N, B, seed, step, cursor=0):
    """(noise_t float32 [N, B, N, 2], noise_a float32 [N, B, 2])."""
    g = gumbel(noise_words(N, B, seed, step, cursor)).astype(np.float32)
    return np.ascontiguousarray(g[:, :, :int(N)]), np.ascontiguousarray(g[:, :, int(N)])
