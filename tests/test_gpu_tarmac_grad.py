"""The training path of the TarMAC actor on the GPU: mdr_tarmac_comm_backward against the dense fp64 gradient under the derived
bound of tests/tarmac_grad_ref.py (every element, no exclusions), its exact corners, the forward's Philox mask, strided operands,
every refusal, mdr_amd.tarmac.band_attention through autograd, and TarMACActor.forward(differentiable=True) end to end on the
recorded reference cases.

End-to-end figures of the first GPU run (profiles/tarmac_grad_README.md): relative L2 error of the parameter gradients against
fp64, largest over a case's tensors, band path on the GPU / float32 dense path on the CPU: f22_n20_c10 1.15e-6 / 6.59e-7,
f22_n6_c0 2.35e-7 / 3.17e-7, f51_n2_c10 3.88e-6 / 9.14e-6, f51_n50_c10_hops2 2.96e-6 / 7.32e-7, f51_n5_c3 1.45e-6 / 1.25e-6; the
largest per-tensor ratio band / yardstick 4.05."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_ref as ar
from tests import tarmac_grad_ref as gr
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = tr.load_cases()
TRAINED = sorted(n for n, c in CASES.items() if c["with_comm"] and c["mode"] == tr.NEIGHBOURS)      # the cases that communicate
# The band path may be at most this factor worse than the float32 dense path on the CPU (the yardstick: existing code, not under
# test), with a floor of 2^-20: the order of summation and the fast exp differ, a wrong gradient is off by O(1).  8: twice the
# largest ratio of the first GPU run (4.05), half of the 16 it may be at most.
E2E_FACTOR, E2E_FLOOR = 8.0, 2.0 ** -20


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _lib():
    import mdr_amd
    return mdr_amd.load_native()


def _workspace(A, K, V):
    n = _lib().mdr_tarmac_comm_backward_workspace_bytes(A, K, V)
    assert n == 16 * A
    return torch.empty(max(n, 16), dtype=torch.uint8, device=DEV)


def _key(prob, seed, step, step_dev, hop):
    return C.c_float(prob), C.c_uint64(seed), C.c_uint64(step), _ptr(step_dev), hop


def _forward(q, k, v, E, N, c, out, K, V, mode=tr.NEIGHBOURS, prob=0.0, seed=0, step=0, step_dev=None, hop=0):
    return _lib().mdr_tarmac_comm(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), E, N, K, V, c, mode,
                                  *_key(prob, seed, step, step_dev, hop), _ptr(out), out.stride(0),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _backward(q, k, v, out, g, dq, dk, dv, ws, E, N, c, K=None, V=None, mode=tr.NEIGHBOURS, prob=0.0, seed=0, step=0, step_dev=None,
              hop=0, q_off=0):
    """mdr_tarmac_comm_backward on 2-D views (rows = agents; the leading dimension is the view's row stride)."""
    K = q.shape[1] if K is None else K
    V = v.shape[1] if V is None else V
    return _lib().mdr_tarmac_comm_backward(_ptr(q, q_off), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), E, N, K, V, c, mode,
                                           *_key(prob, seed, step, step_dev, hop), _ptr(out), out.stride(0), _ptr(g), g.stride(0),
                                           _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), _ptr(ws),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _device(ref):
    return tuple(torch.from_numpy(ref[n].reshape(-1, ref[n].shape[2]).copy()).to(DEV) for n in ("q", "k", "v", "g"))


def _run(shape, ref, **key):
    """Forward, then backward into recycled (0xFF) memory -> (dq, dk, dv, out, the operands)."""
    E, N, c, K, V = shape
    A = E * N
    q, k, v, g = _device(ref)
    out = torch.empty((A, V), dtype=torch.float32, device=DEV)
    assert _forward(q, k, v, E, N, c, out, K, V, **key) == 0
    dq, dk, dv = (torch.empty((A, d), dtype=torch.float32, device=DEV) for d in (K, K, V))
    assert _backward(q, k, v, out, g, dq, dk, dv, _workspace(A, K, V), E, N, c, **key) == 0
    return dq, dk, dv, out, (q, k, v, g)


def _hold_the_bound(what, shape, got, ref):
    E, N = shape[:2]
    for name, t, r, b in zip(("dq", "dk", "dv"), got, ref["grad"], ref["bound"]):
        x = t.cpu().numpy().reshape(E, N, -1)
        assert np.isfinite(x).all(), name
        w = gr.worst(x, r, b)
        print("%s %s: worst |err| / bound = %.3f" % (what, name, w))
        assert w <= 1.0, name


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", gr.GRAD_CASES, ids=str)
def test_backward_holds_the_bound_on_every_element(shape):
    E, N, c, K, V = shape
    ref = gr.reference(shape)
    dq, dk, dv, out, (q, k, v, g) = _run(shape, ref)
    _hold_the_bound(shape, shape, (dq, dk, dv), ref)
    if tr.clamp(c, N) == 0:      # a softmax over the receiver alone
        assert torch.equal(_bits(dv), _bits(g))
        assert not bool(dq.any()) and not bool(dk.any())
    # the same operands, the same bits: nothing is accumulated in an order that could change
    dq2, dk2, dv2 = (torch.empty_like(t) for t in (dq, dk, dv))
    assert _backward(q, k, v, out, g, dq2, dk2, dv2, _workspace(E * N, K, V), E, N, c) == 0
    for a, b in ((dq, dq2), (dk, dk2), (dv, dv2)):
        assert torch.equal(_bits(a), _bits(b))


def test_backward_mode_none_writes_exact_zeros():
    shape = (13, 20, 10, 8, 16)
    E, N, c, K, V = shape
    q, k, v, g = _device(gr.reference(shape))
    out = torch.zeros((E * N, V), dtype=torch.float32, device=DEV)
    grads = [torch.empty((E * N, d), dtype=torch.float32, device=DEV) for d in (K, K, V)]
    assert _backward(q, k, v, out, g, *grads, None, E, N, c, mode=tr.NONE) == 0      # no workspace needed
    for t in grads:
        assert torch.equal(_bits(t), torch.zeros_like(t, dtype=torch.int32))


@pytest.mark.parametrize("shape", gr.DEFECT_CASES, ids=str)
@pytest.mark.parametrize("hop", [0, 1])
def test_backward_redraws_the_forwards_mask(shape, hop):
    E, N, c, K, V = shape
    dev7 = torch.tensor([gr.DEFECT_STEP_DEV], dtype=torch.int32, device=DEV)
    for key in gr.DEFECT_KEYS:
        ref = gr.reference(shape, hop, key)
        dead = ref["dead"]
        kw = dict(prob=gr.DEFECT_PROB, seed=gr.DEFECT_SEED, step=key[0], step_dev=dev7 if key[1] else None, hop=hop)
        dq, dk, dv, out, (q, k, v, g) = _run(shape, ref, **kw)
        _hold_the_bound("%s hop %d step %#x" % (shape, hop, key[0]), shape, (dq, dk, dv), ref)
        # a dead sender's dk and dv hold its own receiver's term only: dv_s = p_ss g_s with p_ss from a call on that pair alone
        clean = gr.reference(shape)
        assert gr.worst(dv.cpu().numpy().reshape(E, N, V), clean["grad"][2], clean["bound"][2]) > 1.0      # and the mask matters
        own = gr.dense_grad(ref["q"], ref["k"], ref["v"], ref["g"], c, dead=dead)
        idx = tr.sender_index(N, c)
        alive = ~dead[:, idx]
        alive[:, :, 0] = True
        s = np.where(alive, np.einsum("enk,enck->enc", ref["q"].astype(np.float64), ref["k"].astype(np.float64)[:, idx]) / np.sqrt(K), -np.inf)
        p_self = 1.0 / np.exp(s - s[:, :, :1]).sum(axis=2)                          # the weight a receiver gives itself
        assert np.abs(own[2] - p_self[:, :, None] * ref["g"])[dead].max() <= 1e-12  # fp64: exactly that one term ...
        got = dv.cpu().numpy().reshape(E, N, V)
        assert (gr.ratio(got, p_self[:, :, None] * ref["g"], ref["bound"][2])[dead] <= 1.0).all()      # ... and so on the GPU
        out64 = tr.band_attention(ref["q"], ref["k"], ref["v"], c, dead=dead)[0]
        t_self = ((ref["g"].astype(np.float64) * (ref["v"] - out64)).sum(axis=2) * p_self / np.sqrt(K))[:, :, None] * ref["q"]
        assert np.abs(own[1] - t_self)[dead].max() <= 1e-12                          # dk_s = ds_ss q_s / sqrt K alone
        assert (gr.ratio(dk.cpu().numpy().reshape(E, N, K), t_self, ref["bound"][1])[dead] <= 1.0).all()


def test_backward_strided_operands_and_result_columns():
    shape = (6, 50, 10, 8, 16)
    E, N, c, K, V = shape
    A = E * N
    q, k, v = (torch.from_numpy(t.reshape(A, -1)).to(DEV) for t in tr.comm_inputs(E, N, K, V))
    g = torch.from_numpy(gr.grad_out(E, N, V).reshape(A, V)).to(DEV)
    out = torch.empty((A, V), dtype=torch.float32, device=DEV)
    assert _forward(q, k, v, E, N, c, out, K, V) == 0
    plain = [torch.empty((A, d), dtype=torch.float32, device=DEV) for d in (K, K, V)]
    ws = _workspace(A, K, V)
    assert _backward(q, k, v, out, g, *plain, ws, E, N, c) == 0
    qkv = torch.cat([q, k, v], dim=1).contiguous()                      # [A][K + K + V]
    og = torch.cat([out, torch.zeros((A, 4), device=DEV), g], dim=1).contiguous()
    wide = torch.full((A, 4 + K + 4 + K + 8 + V + 4), -7.0, dtype=torch.float32, device=DEV)
    cq, ck, cv = 4, 4 + K + 4, 4 + K + 4 + K + 8
    views = (wide[:, cq:cq + K], wide[:, ck:ck + K], wide[:, cv:cv + V])
    assert _backward(qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:], og[:, :V], og[:, V + 4:], *views, ws, E, N, c) == 0
    for a, b in zip(views, plain):
        assert torch.equal(_bits(a), _bits(b))
    keep = torch.ones(wide.shape[1], dtype=torch.bool, device=DEV)
    for c0, d in ((cq, K), (ck, K), (cv, V)):
        keep[c0:c0 + d] = False
    assert bool((wide[:, keep] == -7.0).all())


def test_backward_argument_checks_launch_nothing():
    from mdr_amd import _native as nat
    E, N = 2, 100
    A = E * N
    wide = torch.randn((A, 256), dtype=torch.float32, device=DEV)
    q, k, v = wide[:, :32], wide[:, 32:64], wide[:, 64:144]
    out, g = wide[:, 144:224], wide[:, 176:256]
    res = torch.full((A, 160), -7.0, dtype=torch.float32, device=DEV)
    grads = (res[:, :32], res[:, 32:64], res[:, 64:144])
    ws = torch.full((16 * A,), 0x5A, dtype=torch.uint8, device=DEV)

    def call(c, ws=ws, **kw):
        return _backward(q, k, v, out, g, *grads, ws, E, N, c, **kw)

    assert call(10, K=6, V=16) == nat.MDR_ERR_UNSUPPORTED          # K no multiple of 4
    assert call(10, K=36, V=16) == nat.MDR_ERR_UNSUPPORTED
    assert call(10, K=8, V=68) == nat.MDR_ERR_UNSUPPORTED          # V > 64
    assert call(70, K=8, V=16) == nat.MDR_ERR_UNSUPPORTED          # c = min(70, 99) > 64
    assert call(10, K=8, V=16, q_off=4) == nat.MDR_ERR_INVALID     # a pointer off 16 bytes
    assert call(10, K=8, V=16, hop=4) == nat.MDR_ERR_INVALID
    assert call(10, K=8, V=16, prob=1.5) == nat.MDR_ERR_INVALID
    assert call(10, K=8, V=16, mode=2) == nat.MDR_ERR_INVALID
    assert call(10, K=8, V=16, ws=None) == nat.MDR_ERR_INVALID     # the workspace is missing
    assert _backward(q, k, v, out, g, grads[0], grads[1], res[:, 65:145], ws, E, N, 10, K=8, V=16) == nat.MDR_ERR_INVALID      # a result off 16 bytes
    torch.cuda.synchronize()
    assert bool((res == -7.0).all()) and bool((ws == 0x5A).all())
    assert call(64, K=8, V=16) == 0                                # the widest band itself is served
    assert bool((res[:, :8] != -7.0).all()) and bool((res[:, 32:40] != -7.0).all()) and bool((res[:, 64:80] != -7.0).all())
    assert bool((res[:, 8:32] == -7.0).all()) and bool((res[:, 40:64] == -7.0).all()) and bool((res[:, 80:] == -7.0).all())
    assert not bool((ws == 0x5A).all())


def test_band_attention_through_autograd():
    from mdr_amd.tarmac import band_attention
    shape = (13, 20, 10, 8, 16)
    E, N, c, K, V = shape
    A = E * N
    seed, step, hop = gr.DEFECT_SEED, 5, 1
    ref = gr.reference(shape, hop, gr.DEFECT_KEYS[0])
    q2, k2, v2, g2 = _device(ref)
    # the projections as column views of one packed buffer (read in place), leaves of the graph
    qkv = torch.cat([q2, k2, v2], dim=1).view(E, N, 2 * K + V).contiguous().requires_grad_()
    q, k, v = qkv[:, :, :K], qkv[:, :, K:2 * K], qkv[:, :, 2 * K:]
    out = band_attention(q, k, v, c, defect_prob=gr.DEFECT_PROB, seed=seed, step=step, hop=hop)
    assert out.shape == (E, N, V) and out.grad_fn is not None
    g = g2.view(E, N, V)
    (grad,) = torch.autograd.grad(out, qkv, g, retain_graph=True)
    # the direct ABI call on the same operands
    o2 = torch.empty((A, V), dtype=torch.float32, device=DEV)
    kw = dict(prob=gr.DEFECT_PROB, seed=seed, step=step, hop=hop)
    assert _forward(q2, k2, v2, E, N, c, o2, K, V, **kw) == 0
    assert torch.equal(_bits(out.detach().view(A, V)), _bits(o2))
    direct = [torch.empty((A, d), dtype=torch.float32, device=DEV) for d in (K, K, V)]
    assert _backward(q2, k2, v2, o2, g2, *direct, _workspace(A, K, V), E, N, c, **kw) == 0
    assert torch.equal(_bits(grad.view(A, -1)), _bits(torch.cat(direct, dim=1)))
    _hold_the_bound("autograd %s" % (shape,), shape, direct, ref)
    # a second backward on the retained graph: the same bits
    (again,) = torch.autograd.grad(out, qkv, g, retain_graph=True)
    assert torch.equal(_bits(again), _bits(grad))
    # once differentiable: a double backward raises instead of returning a wrong second derivative
    (first,) = torch.autograd.grad(out, qkv, g, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(first.sum(), qkv)
    # operands that cannot be read in place are copied, not refused
    qt = q2.view(E, N, K).transpose(0, 1).contiguous().transpose(0, 1).requires_grad_()      # [E, N, K] with permuted strides
    o3 = band_attention(qt, k.detach(), v.detach(), c, defect_prob=gr.DEFECT_PROB, seed=seed, step=step, hop=hop)
    assert torch.equal(_bits(o3), _bits(out.detach()))
    (gq,) = torch.autograd.grad(o3, qt, g)
    assert torch.equal(_bits(gq.view(A, K)), _bits(direct[0]))
    with pytest.raises(ValueError):
        band_attention(q.double(), k.double(), v.double(), c)
    with pytest.raises(ValueError):
        band_attention(q, k[:, :, :4], v, c)
    with pytest.raises(ValueError):
        band_attention(q.cpu(), k.cpu(), v.cpu(), c)


def _loss_grads(actor, obs, W, **kw):
    actor.zero_grad()
    obs = obs.detach().clone().requires_grad_()
    p = actor(obs, **kw)
    (p * W).sum().backward()
    grads = {n: w.grad.detach().double().cpu().numpy() for n, w in actor.named_parameters() if w.grad is not None}
    grads["obs"] = obs.grad.detach().double().cpu().numpy()
    return p.detach(), grads


def _rel_l2(got, ref):
    """name -> ||got - ref|| / ||ref|| per parameter tensor.  A tensor whose exact gradient vanishes has no relative error -
    hidden2key's last bias always (a constant added to every key moves all scores of a receiver alike, the softmax does not see
    it), the query and key projections when a receiver hears itself alone - and its fp64 value is rounding noise or 0: where
    ||ref|| is below 1e-6 of the case's largest gradient norm, the error is taken relative to that largest norm instead."""
    assert set(got) == set(ref)
    top = max(np.linalg.norm(r) for r in ref.values())
    assert top > 0
    return {n: float(np.linalg.norm(got[n] - ref[n]) / (np.linalg.norm(ref[n]) if np.linalg.norm(ref[n]) > 1e-6 * top else top)) for n in ref}


@pytest.mark.parametrize("name", TRAINED)
def test_differentiable_forward_end_to_end(name):
    case = CASES[name]
    W = torch.randn(case["probs"].shape, generator=torch.Generator().manual_seed(17))
    cpu = tr.make_actor(case, attention="dense")
    obs = torch.from_numpy(case["obs"])
    _, g64 = _loss_grads(copy.deepcopy(cpu).double(), obs.double(), W.double())
    _, g32 = _loss_grads(cpu, obs, W)                                              # the yardstick: float32 dense on the CPU
    band = tr.make_actor(case, attention="band").to(DEV)
    p, gband = _loss_grads(band, obs.to(DEV), W.to(DEV), differentiable=True)
    yard, got = _rel_l2(g32, g64), _rel_l2(gband, g64)
    worst = max(got, key=lambda n: got[n] / max(yard[n], E2E_FLOOR / E2E_FACTOR))
    print("%s: largest relative L2 error over the %d tensors: band %.3e, float32 dense on the CPU %.3e; largest band / max(yardstick, "
          "floor / factor) = %.3f at %s (band %.3e, yardstick %.3e)"
          % (name, len(got), max(got.values()), max(yard.values()), got[worst] / max(yard[worst], E2E_FLOOR / E2E_FACTOR), worst,
             got[worst], yard[worst]))
    for n in got:
        assert got[n] <= max(E2E_FACTOR * yard[n], E2E_FLOOR), (n, got[n], yard[n])
    # the probabilities: the recorded reference's, and those of the default (no-gradient) forward
    assert ar.contract_ratio(p.cpu().numpy(), case["probs"], False).max() <= 1.0
    with torch.no_grad():
        plain = band(obs.to(DEV))
    assert plain.grad_fn is None and not plain.requires_grad
    assert ar.contract_ratio(p.cpu().numpy(), plain.double().cpu().numpy(), False).max() <= 1.0


def test_default_forward_still_carries_no_gradient():
    case = CASES["f51_n50_c10_hops2"]
    band = tr.make_actor(case, attention="band").to(DEV)
    obs = torch.from_numpy(case["obs"]).to(DEV).requires_grad_()
    p = band(obs)                                      # grad mode on, parameters requiring grad: still the inference path
    assert p.grad_fn is None and not p.requires_grad
    assert torch.equal(p, band(obs, differentiable=False))
    pd = band(obs, differentiable=True)
    assert pd.grad_fn is not None
    # with defects the training path draws the masks of (seed, step, hop), as the inference path does
    noisy = tr.make_actor(case, attention="band", defect_prob=0.3).to(DEV)
    with torch.no_grad():
        a = noisy(obs, seed=77, step=12)
    b = noisy(obs, seed=77, step=12, differentiable=True)
    assert ar.contract_ratio(b.detach().cpu().numpy(), a.double().cpu().numpy(), False).max() <= 1.0
    assert ar.contract_ratio(b.detach().cpu().numpy(), pd.detach().double().cpu().numpy(), False).max() > 100.0
    b[..., 0].sum().backward()
    assert all(w.grad is not None and bool(torch.isfinite(w.grad).all()) for w in noisy.parameters())
