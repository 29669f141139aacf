"""numpy restatement of the device-side minibatch indices (include/mdr_policy.h: mdr_minibatch_permutation, mdr_minibatch_sample),
built on the oracle's Philox4x32-10: the integers the kernels must give, one for one.  ``rounds`` and ``half_bits`` exist so that a
test can build a deliberately wrong variant and see that it gives other integers."""
import numpy as np

from oracle.mdr_oracle import philox4x32_10

TAG_MINIBATCH = 0x4D425031      # "MBP1"
TAG_REPLAY = 0x4D425331         # "MBS1"
M32 = 0xFFFFFFFF


def half_width(n):
    """h = ceil(b / 2) with b = max(1, ceil(log2 n)): the Feistel domain is the 2h-bit integers."""
    b = max(1, (int(n) - 1).bit_length())
    return (b + 1) // 2


def _counter(epoch, cursor, tag):
    epoch = int(epoch) & 0xFFFFFFFFFFFFFFFF
    return ((epoch & M32) + (int(cursor) & M32)) & M32, tag ^ (epoch >> 32)


def permutation(n, seed, epoch, cursor=0, rounds=4, half_bits=None):
    """int64 [n]: element i -> x = i, x = feistel(x) until x < n.  ``cursor`` is the device int32 added to the low word of ``epoch``."""
    n = int(n)
    h = half_width(n) if half_bits is None else int(half_bits)
    mask = np.uint64((1 << h) - 1)
    c2, c3 = _counter(epoch, cursor, TAG_MINIBATCH)
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    x = np.arange(n, dtype=np.uint64)
    out = np.zeros(n, dtype=np.int64)
    todo = np.arange(n)
    while todo.size:
        L, R = x >> np.uint64(h), x & mask
        for r in range(rounds):
            f = philox4x32_10(R, r, c2, c3, k0, k1)[0] & mask
            L, R = R, L ^ f
        x = (L << np.uint64(h)) | R
        done = x < np.uint64(n)
        out[todo[done]] = x[done].astype(np.int64)
        todo, x = todo[~done], x[~done]
    return out


def sample(nb, length, seed, step, cursor=0):
    """int64 [nb]: (word * length) >> 32 with word = .x of Philox on (i lo, i hi, step lo + cursor, TAG_REPLAY ^ step hi)."""
    c2, c3 = _counter(step, cursor, TAG_REPLAY)
    i = np.arange(int(nb), dtype=np.uint64)
    word = philox4x32_10(i & np.uint64(M32), i >> np.uint64(32), c2, c3, int(seed) & M32, (int(seed) >> 32) & M32)[0]
    return ((word * np.uint64(int(length))) >> np.uint64(32)).astype(np.int64)


def chi_square_quantile(p, dof):
    """Wilson-Hilferty: the p quantile of chi-square with ``dof`` degrees of freedom (scipy's where it imports)."""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(p, dof))
    except Exception:
        pass
    # the normal quantile by bisection on erf (p = 0.999 -> 3.0902)
    from math import erf, sqrt
    lo, hi = -10.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * (1.0 + erf(mid / sqrt(2.0))) < p:
            lo = mid
        else:
            hi = mid
    z = 0.5 * (lo + hi)
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * sqrt(2.0 / (9.0 * dof))) ** 3
