"""TarMAC-PPO's centralised critic step on the CPU: tests/tarmac_critic_ref.py held to account (its closed forms against autograd of
the reference's statements in fp64, its bound against fp32 evaluations in two summation orders and torch's, against deliberately wrong
variants, the exactness of z1 and z2 on the grids), the host-side refusals and size functions of mdr_tarmac_critic_*, and the
learner's keyword.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import tarmac_critic_ref as R


def _index(M, B):
    """A minibatch of B out of M stored env-steps: out of order, with repeats once B > 2."""
    idx = (np.arange(B) * 7 + 3) % M
    if B > 2:
        idx[2] = idx[0]
    return idx


def _module(d, dtype):
    from mdr_amd.tarmac import TarMACCritic
    _, N, F = d["state"].shape
    critic = TarMACCritic(N, F, d["W1"].shape[0]).to(dtype)
    with torch.no_grad():
        for p, k in zip(critic.parameters(), R.PARAM_NAMES):
            p.copy_(torch.tensor(np.asarray(d[k]), dtype=dtype))
    return critic


def _autograd(d, index, dtype):
    """agents/tarmac_ppo.py:159-166, 196-204 on the TarMAC_Critic layout -> (value, delta, loss, flat grad) as numpy."""
    critic = _module(d, dtype)
    state, target = torch.tensor(np.asarray(d["state"]), dtype=dtype), torch.tensor(np.asarray(d["target"]), dtype=dtype)
    idx = torch.tensor(index)
    V = critic(state[idx])
    delta = target[idx] - V
    loss = torch.pow(delta, 2).mean(0).mean(0)
    loss.backward()
    return (V.detach().numpy(), delta.detach().numpy(), float(loss.detach()), np.concatenate([p.grad.numpy().reshape(-1) for p in critic.parameters()]))


@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_closed_forms_equal_autograd_of_the_reference_statements(net):
    M, B = 40, 33
    d = R.inputs(M, *net)
    idx = _index(M, B)
    ref = R.evaluate(d, index=idx)
    V, delta, loss, grad = _autograd(d, idx, torch.float64)
    np.testing.assert_allclose(V, ref["value"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(delta, ref["advantage"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(loss, ref["loss"], rtol=1e-12)
    scale = np.abs(ref["grad"]).max()
    np.testing.assert_allclose(grad, ref["grad"], rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_z1_and_z2_are_exact_in_fp32_in_any_order(net):
    d = R.inputs(65, *net)
    ref = R.evaluate(d)
    for perm in (False, True):
        got = R.evaluate(d, dtype=np.float32, perm=perm)
        assert np.array_equal(got["z1"].astype(np.float64), ref["z1"]) and np.array_equal(got["z2"].astype(np.float64), ref["z2"]), perm
    assert (ref["z1"] > 0).mean() > 0.2 and (ref["z2"] > 0).mean() > 0.2      # both masks cut and pass


@pytest.mark.parametrize("B", [1, 17, 65])
@pytest.mark.parametrize("net", R.NETS, ids=str)
def test_fp32_evaluations_stay_inside_the_bound(net, B):
    case = R.reference(B, *net)
    for perm in (False, True):
        got = R.evaluate(case["inputs"], dtype=np.float32, perm=perm)
        for k in R.FLOAT_KEYS:
            assert R.worst(got[k], case["ref"][k], case["bound"][k]) <= 1.0, (k, perm)
    # torch's fp32 autograd order as a third
    V, delta, loss, grad = _autograd(case["inputs"], np.arange(B), torch.float32)
    for k, got in (("value", V), ("advantage", delta), ("loss", loss), ("grad", grad)):
        assert R.worst(got, case["ref"][k], case["bound"][k]) <= 1.0, k


@pytest.mark.parametrize("B", R.ROWS)
@pytest.mark.parametrize("net", R.NETS, ids=str)
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_variants_leave_the_bound_wherever_they_differ(variant, net, B):
    M = B + 3
    d = R.inputs(M, *net)
    idx = _index(M, B)
    ref, bnd = R.evaluate(d, index=idx), R.bound(d, index=idx)
    got = R.evaluate(d, variant=variant, index=idx)
    if np.array_equal(got["grad"], ref["grad"]):      # the variant is the right formula at this shape (one agent, one row, ...)
        N, F, _ = net
        same = dict(mean_B_only=N == 1, sum=B * N == 1, target_not_gathered=B == 1, w3_reversed=N == 1, drop_outputs_past_16=N <= 16,
                    drop_tail_chunk=(N * F) % R.KC == 0, relu0=not ((ref["z1"] == 0).any() or (ref["z2"] == 0).any()))
        assert same.get(variant, False), "the variant must differ here"
        return
    assert R.worst(got["grad"], ref["grad"], bnd["grad"]) > 1.0


def test_every_variant_differs_somewhere():
    """No variant is skipped at every shape: each differs at the reference's shape with 17 rows at least."""
    M, B = 20, 17
    d = R.inputs(M, *R.NETS[5])
    idx = _index(M, B)
    ref = R.evaluate(d, index=idx)
    for variant in R.VARIANTS:
        assert not np.array_equal(R.evaluate(d, variant=variant, index=idx)["grad"], ref["grad"]), variant


# ---- the C calls' host-side refusals and size functions: nothing below reaches a device

def _mlp(K=20 * 51, H1=64, H2=64, O=20, size=None, ptr=0x1000):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, K, H1, H2, O, *([ptr] * 6))


def test_signatures_match_the_header():
    lib = nat.load()
    assert len(lib.mdr_tarmac_critic_value.argtypes) == 8 and len(lib.mdr_tarmac_critic_grad.argtypes) == 13
    assert lib.mdr_tarmac_critic_grad_floats.restype is C.c_int64 and lib.mdr_tarmac_critic_workspace_bytes.restype is C.c_int64


def test_size_functions():
    lib = nat.load()
    assert lib.mdr_tarmac_critic_grad_floats(C.byref(_mlp())) == 64 * 1020 + 64 + 64 * 64 + 64 + 20 * 64 + 20
    assert lib.mdr_tarmac_critic_grad_floats(C.byref(_mlp(K=50 * 51, O=50))) == 64 * 2550 + 64 + 64 * 64 + 64 + 50 * 64 + 50
    assert lib.mdr_tarmac_critic_grad_floats(C.byref(_mlp(K=5 * 63, H1=97, H2=113, O=5))) == 97 * 315 + 97 + 113 * 97 + 113 + 5 * 113 + 5
    assert lib.mdr_tarmac_critic_grad_floats(C.byref(_mlp(K=4096, H1=256, H2=256, O=64))) > 0
    for bad in (_mlp(K=4097, O=1), _mlp(H1=257), _mlp(H2=257), _mlp(K=65 * 4, O=65), _mlp(O=0), _mlp(O=-1), _mlp(K=1021), _mlp(size=8),
                _mlp(K=0), _mlp(H1=0), _mlp(H2=-4)):
        assert lib.mdr_tarmac_critic_grad_floats(C.byref(bad)) == -1
    assert lib.mdr_tarmac_critic_grad_floats(None) == -1
    # rows padded to 16: h1, dz1, h2, dz2 [Bp][64], dV [Bp][32], the loss terms [Bp]
    assert lib.mdr_tarmac_critic_workspace_bytes(C.byref(_mlp()), 64, 0) == 64 * (4 * 64 + 32 + 1) * 4
    assert lib.mdr_tarmac_critic_workspace_bytes(C.byref(_mlp()), 65, 2) == 80 * (4 * 64 + 32 + 1) * 4
    assert lib.mdr_tarmac_critic_workspace_bytes(C.byref(_mlp(K=5 * 63, H1=97, H2=113, O=5)), 17, 0) == 32 * (2 * 112 + 2 * 128 + 16 + 1) * 4
    assert lib.mdr_tarmac_critic_workspace_bytes(C.byref(_mlp()), 0, 0) >= 16
    for net, B, mw in ((_mlp(), -1, 0), (_mlp(), 16, -1), (_mlp(H1=257), 16, 0), (_mlp(K=1021), 16, 0), (_mlp(size=8), 16, 0)):
        assert lib.mdr_tarmac_critic_workspace_bytes(C.byref(net), B, mw) == -1


def test_calls_refuse_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
    critic = _mlp()

    def vcall(c=critic, state=p, ld=1020, B=16, mw=0, value=p):
        return lib.mdr_tarmac_critic_value(C.byref(c) if c is not None else None, state, ld, None, B, mw, value, None)

    def gcall(c=critic, state=p, ld=1020, target=p, B=16, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_tarmac_critic_grad(C.byref(c) if c is not None else None, state, ld, target, None, B, mw, ws, grad, loss, None, None, None)

    invalid = (dict(c=None), dict(state=None), dict(ld=1019), dict(B=-1), dict(mw=-1), dict(c=_mlp(size=8)), dict(c=_mlp(ptr=None)), dict(c=_mlp(O=0)),
               dict(c=_mlp(O=-2)), dict(c=_mlp(K=1021)), dict(c=_mlp(K=-1020)), dict(c=_mlp(H1=0)), dict(c=_mlp(H2=-1)),
               dict(c=_mlp(K=4097, O=1), ld=4097 - 1))
    unsupported = (dict(c=_mlp(K=4097, O=1), ld=4097), dict(c=_mlp(H1=257)), dict(c=_mlp(H2=257)), dict(c=_mlp(K=65 * 4, O=65)))
    for kw in invalid + (dict(value=None),):
        assert vcall(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in invalid + (dict(target=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ws=C.c_void_p(0x1004))):
        assert gcall(**kw) == nat.MDR_ERR_INVALID, kw
    for kw in unsupported:
        assert vcall(**kw) == nat.MDR_ERR_UNSUPPORTED and gcall(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert vcall(B=0) == nat.MDR_OK      # zero rows: nothing to launch


# ---- the Python layer without a device

def test_cpu_critic_is_refused_and_the_learner_reads_the_keyword():
    from mdr_amd import tarmac_ppo
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    critic = TarMACCritic(3, 5, 16)
    assert not tarmac_ppo.critic_supported(critic) and "GPU" in tarmac_ppo._critic_refusal(critic)
    assert "TarMACCritic" in tarmac_ppo._critic_refusal(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="GPU"):
        tarmac_ppo.critic_value(critic, torch.zeros((4, 3, 5)))
    with pytest.raises(ValueError, match="GPU"):
        tarmac_ppo.critic_loss_backward(critic, torch.zeros((4, 3, 5)), torch.zeros((4, 3)))
    actor = TarMACActor(5, 4, 4, 8)
    prop = {"lr_actor": 1e-3, "lr_critic": 3e-3, "clip_param": 0.2, "max_grad_norm": 0.5, "ppo_update_time": 2, "batch_size": 16}
    learner = tarmac_ppo.TarMACPPOLearner.from_config(prop, actor, critic, backend="torch")
    assert learner.critic_backend == "torch" and not learner.critic_uses_kernels(16)
    auto = tarmac_ppo.TarMACPPOLearner.from_config(prop, actor, critic, backend="torch", critic_backend="auto")
    assert auto.critic_backend == "auto" and not auto.critic_uses_kernels(16)      # CPU parameters: auto falls back to torch
    with pytest.raises(ValueError, match="critic_backend='hip'"):
        tarmac_ppo.TarMACPPOLearner(actor, critic, 1e-3, 1e-3, backend="torch", critic_backend="hip")
    with pytest.raises(ValueError, match="critic_backend must"):
        tarmac_ppo.TarMACPPOLearner(actor, critic, 1e-3, 1e-3, backend="torch", critic_backend="cuda")
