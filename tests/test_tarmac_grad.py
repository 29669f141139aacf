"""The restatement and the rounding bound of tests/tarmac_grad_ref.py, judged on the CPU on every input tests/test_gpu_tarmac_grad.py
uses: the two-pass formulas in fp64 equal the dense fp64 gradient, the same formulas in float32 stay inside the bound on every
element, and each wrong variant a kernel could plausibly be leaves it for most agents - so the bound is neither too tight for a
right kernel nor loose enough to pass a wrong one.  Plus the Python surface that needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tarmac_grad_ref as gr
from tests import tarmac_ref as tr

# every (shape, hop, key) the GPU test runs
PLAIN = [(shape, None, None) for shape in gr.GRAD_CASES]
DEFECT = [(shape, hop, key) for shape in gr.DEFECT_CASES for hop in (0, 1) for key in gr.DEFECT_KEYS]


def _breached(got, ref, bound):
    """bool [E, N]: the agent has an element outside the bound (a NaN is outside)."""
    return ~(gr.ratio(got, ref, bound) <= 1.0).all(axis=2)


@pytest.mark.parametrize("case", PLAIN + DEFECT, ids=str)
def test_two_pass_formulas_equal_the_dense_gradient_in_fp64(case):
    shape, hop, key = case
    ref = gr.reference(*case)
    got = gr.band_grad(ref["q"], ref["k"], ref["v"], ref["g"], shape[2], dead=ref["dead"])
    for name, a, b in zip(("dq", "dk", "dv"), got, ref["grad"]):
        assert np.abs(a - b).max() <= 1e-12, name
    if ref["dead"] is not None:
        assert 0.15 < ref["dead"].mean() < 0.45


@pytest.mark.parametrize("case", PLAIN + DEFECT, ids=str)
def test_float32_evaluation_stays_inside_the_bound_on_every_element(case):
    shape, hop, key = case
    ref = gr.reference(*case)
    got = gr.band_grad(ref["q"], ref["k"], ref["v"], ref["g"], shape[2], dead=ref["dead"], dtype=np.float32)
    for name, a, b, bound in zip(("dq", "dk", "dv"), got, ref["grad"], ref["bound"]):
        assert a.dtype == np.float32 and np.isfinite(a).all()
        w = gr.worst(a, b, bound)
        print("%s %s: worst |err| / bound = %.3f" % (case, name, w))
        assert w <= 1.0, name


# with no sender but the receiver itself (N = 1, c = 0) every variant IS the gradient: dq = dk = 0, dv = g
@pytest.mark.parametrize("case", [x for x in PLAIN + DEFECT if tr.clamp(x[0][2], x[0][1]) > 0], ids=str)
def test_wrong_variants_leave_the_bound(case):
    shape, hop, key = case
    E, N, c, K, V = shape
    cc = tr.clamp(c, N)
    ref = gr.reference(*case)
    args = (ref["q"], ref["k"], ref["v"], ref["g"], c)
    (rq, rk, rv), (bq, bk, bv) = ref["grad"], ref["bound"]
    half = E * N / 2
    if cc % 2 and cc < N - 1:                                             # (a) the sender-major offsets not mirrored
        _, dk, dv = gr.band_grad(*args, dead=ref["dead"], mirrored=False)
        assert max(_breached(dk, rk, bk).sum(), _breached(dv, rv, bv).sum()) > half
    dq, dk, _ = gr.band_grad(*args, dead=ref["dead"], use_delta=False)    # (b) delta dropped
    assert max(_breached(dq, rq, bq).sum(), _breached(dk, rk, bk).sum()) > half
    dq, dk, _ = gr.band_grad(*args, dead=ref["dead"], scale=False)        # (c) the 1 / sqrt K missing
    assert _breached(dq, rq, bq).sum() > half and _breached(dk, rk, bk).sum() > half
    if ref["dead"] is not None:                                           # (d) defects ignored in the sender-major pass
        _, dk, dv = gr.band_grad(*args, dead=ref["dead"], sender_defects=False)
        d = ref["dead"]
        assert _breached(dk, rk, bk)[d].sum() > d.sum() / 2 and _breached(dv, rv, bv)[d].sum() > d.sum() / 2
        assert not _breached(dv, rv, bv)[~d].any()                        # and only there


@pytest.mark.parametrize("shape", [(5, 6, 3, 8, 16), (13, 20, 10, 8, 16)], ids=str)
def test_closed_form_equals_autograd_of_the_actors_dense_formula(shape):
    """The dense closed form is itself checked against torch autograd of the formula TarMACActor.dense_logits evaluates."""
    E, N, c, K, V = shape
    ref = gr.reference(shape)
    dead = tr.dead_mask(E, N, 0.3, 3, 1)
    for d in (None, dead):
        q, k, v = (torch.from_numpy(ref[n].copy()).double().requires_grad_() for n in ("q", "k", "v"))
        mask = torch.from_numpy(np.ascontiguousarray(gr.dense_mask(E, N, c, d)))
        scores = torch.matmul(q, k.transpose(-2, -1)) / np.sqrt(K)
        e = torch.exp(scores - scores.max(dim=-1, keepdim=True)[0]) * mask.double()
        out = torch.matmul(e / e.sum(dim=-1, keepdim=True), v)
        out.backward(torch.from_numpy(ref["g"].copy()).double())
        for a, b in zip((q.grad, k.grad, v.grad), gr.dense_grad(ref["q"], ref["k"], ref["v"], ref["g"], c, dead=d)):
            assert np.abs(a.numpy() - b).max() <= 1e-12


def test_mode_none_and_the_receiver_alone():
    E, N, K, V = 3, 20, 8, 16
    q, k, v = tr.comm_inputs(E, N, K, V)
    g = gr.grad_out(E, N, V)
    for fn in (gr.band_grad, gr.dense_grad, gr.grad_bound):
        assert all(not x.any() for x in fn(q, k, v, g, 10, mode=tr.NONE))
    dq, dk, dv = gr.band_grad(q, k, v, g, 0, dtype=np.float32)
    assert np.array_equal(dv, g) and not dq.any() and not dk.any()


def test_the_library_exports_the_backward_and_sizes_its_workspace():
    import mdr_amd
    lib = mdr_amd.load_native()
    assert lib.mdr_tarmac_comm_backward_workspace_bytes(4096 * 1024, 8, 16) == 16 * 4096 * 1024
    assert lib.mdr_tarmac_comm_backward_workspace_bytes(0, 8, 16) == 0
    assert lib.mdr_tarmac_comm_backward_workspace_bytes(-1, 8, 16) == -1
    # host-side refusals come before any launch: no device needed
    args = [None, 8, None, 8, None, 16, 1, 4, 8, 16, 2, 0, C.c_float(0.0), 0, 0, None, 0, None, 16, None, 16, None, 8, None, 8, None, 16, None, None]
    assert lib.mdr_tarmac_comm_backward(*args) == -1


def test_band_attention_validates_its_operands_and_forward_takes_the_flag():
    from mdr_amd.tarmac import TarMACActor, band_attention
    q, v = torch.zeros((2, 5, 8)), torch.zeros((2, 5, 16))
    with pytest.raises(ValueError):
        band_attention(q, q, v, 3)                                        # CPU tensors
    with pytest.raises(ValueError):
        band_attention(q.double(), q.double(), v.double(), 3)
    with pytest.raises(ValueError):
        band_attention(q[0], q[0], v[0], 3)
    # differentiable=True on CPU tensors falls through to the dense path, which carries a gradient anyway
    torch.manual_seed(0)
    actor = TarMACActor(6, number_agents_comm=3, num_hops=2)
    obs = torch.randn((2, 5, 6), requires_grad=True)
    p = actor(obs, differentiable=True)
    assert p.grad_fn is not None and torch.equal(p, actor(obs))
    p[..., 0].sum().backward()
    assert obs.grad is not None and all(w.grad is not None for w in actor.parameters())
