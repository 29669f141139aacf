"""A plain fp64 restatement of what the fused actor kernels compute (include/mdr_policy.h): the Linear/ReLU/Linear/ReLU/Linear
forward with a running rounding-error bound for the logit difference, and the Philox draw behind every sampled action.  numpy on
the CPU only; tests/test_gpu_actor_forms.py holds every kernel form to it.

The error bound is derived, never fitted to what a kernel returns.  A layer y = W x + b of fan-in k, evaluated as a chain of k
fp32 fused multiply-adds that starts from the bias, is off by at most gamma_k (|W| |x| + |b|), gamma_k = k u / (1 - k u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); (k + 2) u leaves room for the second-order term and for the
one rounding of the head's weight difference W3[0] - W3[1], which the host takes in fp32.  An error err_in already on x passes
through as |W| err_in, and ReLU is 1-Lipschitz.  The bf16x3 layout feeds the matrix cores operands split into a bf16 head and tail
and drops the tail x tail product: DESIGN.md states that unit as 2^-16 of every product (head + tail keep an operand to 2^-18 each,
the dropped product is 2^-18 of the whole: 3 * 2^-18 < 2^-16), on top of the fp32 accumulation."""
import numpy as np

from oracle.mdr_oracle import philox4x32_10

TAG_ACTION = 0x41435431             # csrc/mdr_policy.hip
U_FP32 = 2.0 ** -24
U_BF16X3 = 2.0 ** -16               # DESIGN.md, k_actor_sample_bf16: what the head + tail split loses of a product
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)      # 0x1.fffffep-1: the largest float below 1
BF16X3 = 2                          # mdr_actor_layout

# the project's contract for probabilities (tests/test_gpu_policy.py): |p - ref| <= rtol |ref| + atol
CONTRACT = {False: (1e-5, 2e-6), True: (2e-3, 2e-5)}      # keyed by "layout is bf16x3"
BF16_MEAN_ABS = 5e-6


def _f64(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def module_weights(actor):
    """(w1, b1, w2, b2, w3, b3) of an ActorMLP as float64 numpy arrays."""
    fc = list(actor.fc)
    return tuple(_f64(t) for lin in fc for t in (lin.weight, lin.bias))


def _layer(w, b, x, err, product_unit):
    k = w.shape[1]
    aw = np.abs(w)
    y = x @ w.T + b
    mag = np.abs(x) + err
    acc = (k + 2) * U_FP32
    err_out = err @ aw.T + acc * (mag @ aw.T + np.abs(b)) + product_unit * (mag @ aw.T)
    return y, err_out


def forward64(w1, b1, w2, b2, w3, b3, rows, layout=0):
    """-> (d, p0, p1, bound): d = logit0 - logit1 in fp64, p0 = 1 / (1 + exp(-d)), p1 = 1 / (1 + exp(d)) and the running bound on
    |d_kernel - d| for a kernel of this layout (module docstring)."""
    w1, b1, w2, b2, w3, b3, x = (_f64(t) for t in (w1, b1, w2, b2, w3, b3, rows))
    unit = U_BF16X3 if layout == BF16X3 else 0.0
    err = np.zeros_like(x)
    h1, err = _layer(w1, b1, x, err, unit)
    h1 = np.maximum(h1, 0.0)
    h2, err = _layer(w2, b2, h1, err, unit)
    h2 = np.maximum(h2, 0.0)
    d, bound = _layer((w3[0] - w3[1])[None, :], np.array([b3[0] - b3[1]]), h2, err, 0.0)      # the head runs on fp32 fmas in every layout
    d, bound = d[:, 0], bound[:, 0]
    with np.errstate(over="ignore"):
        p0 = 1.0 / (1.0 + np.exp(-d))
        p1 = 1.0 / (1.0 + np.exp(d))
    return d, p0, p1, bound


def draw_word(agent, seed, step, step_dev=0):
    """The 32 random bits behind agent's action (include/mdr_policy.h): word 0 of Philox4x32-10 with key = (seed lo, seed hi) and
    counter = (agent lo, agent hi, (step lo + step_dev) mod 2^32, TAG_ACTION ^ step hi): `step_dev` is added to the low word of
    `step` alone and never carries into the high one."""
    agent = np.asarray(agent, dtype=np.uint64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    c2 = ((step & 0xFFFFFFFF) + (int(step_dev) & 0xFFFFFFFF)) & 0xFFFFFFFF
    c3 = TAG_ACTION ^ (step >> 32)
    x = philox4x32_10(agent & np.uint64(0xFFFFFFFF), agent >> np.uint64(32), c2, c3, seed & 0xFFFFFFFF, seed >> 32)[0]
    return x.astype(np.uint32)


def uniform_of(word, clamp=True):
    """u = min(((float)(x >> 8) + 0.5f) * 2^-24, 0x1.fffffep-1f), every operation in float32 as the kernel rounds it.  Without the
    clamp x >> 8 == 0xFFFFFF gives 1.0f: 16777215.5 ties to even."""
    hi = (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)      # < 2^24: exact
    u = (hi + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return np.minimum(u, U_MAX) if clamp else u


def draw_u(agent, seed, step, step_dev=0):
    return uniform_of(draw_word(agent, seed, step, step_dev))


def kernel_logit_difference(probs):
    """d_kernel = log(p0 / p1) from the two stored float32 probabilities (fp64 arithmetic), and where it is defined: both normal."""
    p = np.asarray(probs, dtype=np.float32)
    tiny = np.finfo(np.float32).tiny
    normal = (p[:, 0] >= tiny) & (p[:, 1] >= tiny)
    p64 = p.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.log(p64[:, 0]) - np.log(p64[:, 1])
    return d, normal


def expected_action(u, p0_kernel, greedy, d_kernel):
    """Categorical(probs).sample() by inversion - u < p0 ? 0 : 1 on the kernel's own float32 p0 - or, greedy, the argmax that keeps
    the first maximum: d >= 0 ? 0 : 1."""
    if greedy:
        return np.where(np.asarray(d_kernel) >= 0.0, 0, 1).astype(np.uint8)
    return np.where(np.asarray(u, dtype=np.float32) < np.asarray(p0_kernel, dtype=np.float32), 0, 1).astype(np.uint8)


def contract_ratio(p_kernel, p64, bf16):
    """|p_kernel - p64| / (rtol |p64| + atol), elementwise: <= 1 meets the contract."""
    rtol, atol = CONTRACT[bool(bf16)]
    p_kernel = np.asarray(p_kernel, dtype=np.float64)
    return np.abs(p_kernel - p64) / (rtol * np.abs(p64) + atol)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- the inputs of tests/test_gpu_actor_forms.py, built on the CPU so that tests/test_actor_forms.py can judge them without a kernel

SPARSE_KEEP = 8


def make_actor(F, layers, seed, scale, keep=None):
    """An ActorMLP (CPU) with torch's default init times `scale` and biases uniform in +-0.5, as tests/test_gpu_policy.py builds
    its actors.  `keep`: only about that many weights per unit of the two hidden layers stay (rescaled to the same variance of the
    pre-activations).  The running bound grows with sum |w| |x| while the logit difference grows with |sum w x|: a dense 128-127-127
    network loses a factor ~11 per layer to cancellation, so the bound alone covers 1-3 % of its agents whatever the input scale
    (bound and logits scale together); with 8 weights per unit it covers under 0.5 %, which is what the greedy check's 1 % cap needs."""
    import torch
    from mdr_amd.rollout import ActorMLP
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.manual_seed(seed)
    actor = ActorMLP(F, 2, layers)
    with torch.no_grad():
        for lin in actor.fc:
            lin.weight.mul_(scale)
            lin.bias.uniform_(-0.5, 0.5, generator=g)
        if keep is not None:
            for lin in list(actor.fc)[:2]:
                k = lin.weight.shape[1]
                if k > keep:
                    mask = torch.rand(lin.weight.shape, generator=g) < keep / k
                    lin.weight.mul_(mask * (k / keep) ** 0.5)
    return actor


def rows_inputs(F, A, seed):
    """The on-rows inputs: N(0, 1.5^2) float32 rows on the CPU (tests/test_gpu_policy.py draws its rows with factors 1 and 2).
    Larger rows are no option: at eight times the size a torch fp32 forward itself misses the fp32 contract against fp64 (1.1 of
    it), so the contract could no longer tell a wrong kernel from an unlucky one."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((A, F), generator=g) * 1.5
