"""mdr_mlp_actor_sample and FusedMLPActor without a GPU: what the C entry refuses before any launch, what ``refusal`` says about a
module, the opt-in switches, and - judged on the CPU - the inputs tests/test_gpu_mlp_actor.py holds the kernel to."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from mdr_amd import _native as nat
from tests import actor_ref as ar
from tests import mlp_actor_cases as mc


def _mlp(K=51, H1=256, H2=256, O=2, size=None, ptr=0x1000):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, K, H1, H2, O, *([ptr] * 6))


# the calls the C entry refuses, shared with the GPU test that checks they leave the outputs alone: (keywords, status)
REFUSED = [
    (dict(K=129, ld=129), nat.MDR_ERR_UNSUPPORTED), (dict(H1=257), nat.MDR_ERR_UNSUPPORTED), (dict(H2=257), nat.MDR_ERR_UNSUPPORTED),
    (dict(O=1), nat.MDR_ERR_UNSUPPORTED), (dict(O=3), nat.MDR_ERR_UNSUPPORTED),
    (dict(ld=50), nat.MDR_ERR_INVALID), (dict(obs=None), nat.MDR_ERR_INVALID), (dict(action=None), nat.MDR_ERR_INVALID),
    (dict(size=0), nat.MDR_ERR_INVALID),
]


def refused_call(lib, obs, action, a_prob, probs, A=16, ld=51, K=51, H1=256, H2=256, O=2, size=None, ptr=0x1000, mw=0, stream=None):
    """One call of the entry point with pointers as integers (None: NULL); a refused call dereferences none of them."""
    desc = _mlp(K, H1, H2, O, size, ptr)
    return lib.mdr_mlp_actor_sample(C.byref(desc), obs, ld, A, C.c_uint64(1), C.c_uint64(2), None, 0, mw, action, a_prob, probs, stream)


def test_signature_matches_the_header():
    lib = nat.load()
    assert "mdr_mlp_actor_sample" in nat.EXPORTS and len(lib.mdr_mlp_actor_sample.argtypes) == 13
    assert nat.MDR_ABI_VERSION == 5 == lib.mdr_abi_version()


def test_the_entry_point_refuses_on_the_host():
    lib = nat.load()
    p = 0x1000      # never dereferenced: every call below returns before a launch
    for kw, status in REFUSED:
        kw = dict(kw)
        obs, action = kw.pop("obs", p), kw.pop("action", p)
        assert refused_call(lib, obs, action, p, p, **kw) == status, kw
    for kw in (dict(A=-1), dict(mw=-1), dict(ptr=None)):
        assert refused_call(lib, p, p, p, p, **kw) == nat.MDR_ERR_INVALID, kw
    assert lib.mdr_mlp_actor_sample(None, p, 51, 16, C.c_uint64(1), C.c_uint64(2), None, 0, 0, p, p, p, None) == nat.MDR_ERR_INVALID
    for kw in (dict(K=0), dict(H1=0), dict(H2=0)):
        assert refused_call(lib, p, p, p, p, **kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert refused_call(lib, p, p, None, None, A=0) == nat.MDR_OK      # no agents: nothing to launch


class _NoBias(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.ModuleList([nn.Linear(51, 256), nn.Linear(256, 256, bias=False), nn.Linear(256, 2)])


class _FourLayers(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.ModuleList([nn.Linear(51, 64), nn.Linear(64, 64), nn.Linear(64, 64), nn.Linear(64, 2)])


def test_refusal_and_supported_on_cpu_modules():
    from mdr_amd.maddpg import DDPGNetworkMLP
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import ActorMLP
    on_cpu = FusedMLPActor.refusal(DDPGNetworkMLP(51, 2, 256))
    assert on_cpu is not None and "GPU" in on_cpu and not FusedMLPActor.supported(DDPGNetworkMLP(51, 2, 256))
    with pytest.raises(ValueError, match="GPU"):
        FusedMLPActor(DDPGNetworkMLP(51, 2, 256))
    for net, word in ((ActorMLP(129, 2, (256, 256)), "129"), (ActorMLP(51, 2, (257, 256)), "257"), (ActorMLP(51, 2, (256, 300)), "300"),
                      (ActorMLP(51, 3, (256, 256)), "3 outputs"), (DDPGNetworkMLP(51, 1, 256), "1 outputs"),
                      (_NoBias(), "three biased Linear"), (_FourLayers(), "three biased Linear"), (nn.Linear(51, 2), "three biased Linear"),
                      (nn.Sequential(nn.Linear(51, 256), nn.ReLU(), nn.Linear(256, 2)), "three biased Linear")):
        why = FusedMLPActor.refusal(net)
        assert why is not None and word in why, (type(net).__name__, why)
        assert not FusedMLPActor.supported(net)
    broken = ActorMLP(51, 2, (256, 256))
    broken.fc[1] = nn.Linear(128, 256)
    assert "chain" in FusedMLPActor.refusal(broken)


def test_unknown_backends_raise():
    from mdr_amd.maddpg import DDPGNetworkMLP, GreedyDDPGActor, train_maddpg
    from mdr_amd.rollout import collect_maddpg_transitions
    actor = DDPGNetworkMLP(51, 2, 256)
    with pytest.raises(ValueError, match="actor_backend"):
        collect_maddpg_transitions(None, actor, 1, actor_backend="bogus")
    with pytest.raises(ValueError, match="actor_backend"):
        collect_maddpg_transitions(None, actor, 1, actor_backend="auto")      # no "auto": nothing was measured to choose by
    with pytest.raises(ValueError, match="actor_backend"):
        train_maddpg(None, types.SimpleNamespace(actor=actor), 1, actor_backend="bogus")
    with pytest.raises(ValueError, match="backend"):
        GreedyDDPGActor(actor, backend="bogus")
    with pytest.raises(ValueError, match="GPU"):      # a net the kernel does not take: the refusal's text
        collect_maddpg_transitions(None, actor, 1, actor_backend="hip")
    with pytest.raises(ValueError, match="GPU"):
        GreedyDDPGActor(actor, backend="hip")
    assert GreedyDDPGActor(actor).backend == "torch"


@pytest.mark.parametrize("shape", mc.SHAPES, ids=mc.shape_id)
def test_gpu_case_inputs_keep_the_fp32_reference_inside_the_contract(shape):
    """The inputs of the GPU cases, judged without a kernel: on 4096 rows at most 1 % of the agents have an fp64 logit difference
    inside forward64's bound (the greedy check's cap), a torch fp32 forward of the same module stays inside the fp32 contract (so a
    kernel that exceeds it is wrong, not unlucky).  The spread of p0 is printed."""
    actor = mc.make_actor(shape)
    rows = mc.rows(shape, 4096)
    d64, p0, p1, bound = ar.forward64(*ar.module_weights(actor), rows.numpy(), layout=0)
    unclear = float((np.abs(d64) <= bound + 8.0 * ar.ulp32(d64)).mean())
    with torch.no_grad():
        ref = actor(rows).numpy()      # ActorMLP ends in the softmax
    ratio = float(np.maximum(ar.contract_ratio(ref[:, 0], p0, False), ar.contract_ratio(ref[:, 1], p1, False)).max())
    print("MLP_ACTOR_INPUTS %s unclear=%.5f torch_fp32=%.4f p0=[%.4f, %.4f]" % (mc.shape_id(shape), unclear, ratio, p0.min(), p0.max()))
    assert unclear <= 0.01
    assert ratio <= 1.0
