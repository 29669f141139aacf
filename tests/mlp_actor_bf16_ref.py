"""What mdr_mlp_actor_sample_bf16x3 computes (include/mdr_policy.h, csrc/mdr_mlp_actor_bf16.hip), restated in numpy on the CPU: both
hidden layers as the three products of operands split into a bf16 head and tail (tests/tarmac_bf16_ref.split), everything else - the
biases, ReLU, the head as one dot with W3[0] - W3[1], the two-logit softmax - in float32.  Switches: the dtype the products are
accumulated in (float32 as the kernel, or float64: the same arithmetic without any accumulation order), and the three wrong variants
that drop a cross term.  Nothing here is fitted to what a kernel returns."""
import numpy as np

from tests.tarmac_bf16_ref import split

VARIANTS = {"no Wl.xh": dict(wl_xh=False), "no Wh.xl": dict(wh_xl=False), "heads only": dict(wl_xh=False, wh_xl=False)}


def _hidden(w, b, x, acc, wl_xh, wh_xl):
    """relu(b + Wh xh [+ Wl xh] [+ Wh xl]) accumulated in `acc`, returned in float32: what the kernel's fp32 accumulators hold."""
    wh, wl = (t.astype(acc) for t in split(w))
    xh, xl = (t.astype(acc) for t in split(x))
    y = b.astype(acc) + xh @ wh.T
    if wl_xh:
        y = y + xh @ wl.T
    if wh_xl:
        y = y + xl @ wh.T
    return np.maximum(y.astype(np.float32), np.float32(0))


def forward(weights, rows, acc=np.float32, wl_xh=True, wh_xl=True):
    """(w1, b1, w2, b2, w3, b3) as actor_ref.module_weights returns them, rows [A, F] -> float32 probabilities [A, 2].
    ``acc``: np.float32 or np.float64.  ``wl_xh=False`` / ``wh_xl=False``: the wrong variants without that cross term; both False:
    heads only."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(t, dtype=np.float32) for t in weights)
    x = np.asarray(rows, dtype=np.float32)
    h = _hidden(w1, b1, x, acc, wl_xh, wh_xl)
    h = _hidden(w2, b2, h, acc, wl_xh, wh_xl)
    wd, bd = w3[0] - w3[1], b3[0] - b3[1]      # rounded to float32, as the kernel takes them
    d = (h.astype(acc) @ wd.astype(acc) + acc(bd)).astype(np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        return np.stack([one / (one + np.exp(-d)), one / (one + np.exp(d))], axis=-1).astype(np.float32)
