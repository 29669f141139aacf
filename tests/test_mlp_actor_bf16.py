"""mdr_mlp_actor_sample_bf16x3 without a GPU: the arithmetic the header states, emulated in numpy (tests/mlp_actor_bf16_ref.py) on the
cases of tests/mlp_actor_cases.py, meets the project's bf16x3 contract against the fp64 forward of tests/actor_ref.py - and the three
forwards that drop a cross term do not, so the GPU test that holds the kernel to the same contract can tell them apart.  Then what
the entry point and ``FusedMLPActor(precision=...)`` refuse on the host."""
import numpy as np
import pytest

from mdr_amd import _native as nat
from tests import actor_ref as ar
from tests import mlp_actor_bf16_ref as br
from tests import mlp_actor_cases as mc
from tests.test_mlp_actor import REFUSED, _mlp

BATCHES = (17, 1029)
_cache = {}


def _case(shape, A):
    """(weights, rows, fp64 logit difference, fp64 probabilities [A, 2], limit on the logit difference): computed once per case."""
    key = (shape, A)
    if key not in _cache:
        weights = ar.module_weights(mc.make_actor(shape))
        rows = mc.rows(shape, A).numpy()
        d64, p0, p1, bound = ar.forward64(*weights, rows, layout=ar.BF16X3)
        _cache[key] = (weights, rows, d64, np.stack([p0, p1], 1), bound + 8.0 * ar.ulp32(d64))
    return _cache[key]


@pytest.mark.parametrize("A", BATCHES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=mc.shape_id)
def test_the_stated_arithmetic_meets_the_bf16x3_contract(shape, A):
    """Accumulated in float32 (as the kernel) and in float64 (no accumulation order at all): the contract ratio, the mean absolute
    error and the logit difference against forward64(layout=BF16X3)'s derived bound + 8 ulp; and, of the fp64 reference alone, the
    share of agents whose logit difference lies inside that bound - the cap of the GPU test's greedy check."""
    weights, rows, d64, p64, limit = _case(shape, A)
    unclear = float((np.abs(d64) <= limit).mean())
    for acc in (np.float32, np.float64):
        p = br.forward(weights, rows, acc=acc)
        ratio = float(ar.contract_ratio(p, p64, True).max())
        mean_abs = float(np.abs(p.astype(np.float64) - p64).mean())
        dk, normal = ar.kernel_logit_difference(p)
        dratio = float((np.abs(dk[normal] - d64[normal]) / limit[normal]).max())
        print("MLP_ACTOR_BF16_EMU %s A=%d acc=%s contract=%.4f mean_abs=%.3e dbound=%.5f unclear=%.5f"
              % (mc.shape_id(shape), A, np.dtype(acc).name, ratio, mean_abs, dratio, unclear))
        assert ratio <= 1.0
        assert mean_abs < ar.BF16_MEAN_ABS
        assert normal.all() and dratio <= 1.0
    assert unclear <= 0.01


@pytest.mark.parametrize("A", BATCHES)
@pytest.mark.parametrize("variant", sorted(br.VARIANTS))
@pytest.mark.parametrize("shape", [s for s in mc.SHAPES if s != (1, (1, 1))], ids=mc.shape_id)
def test_a_forward_without_a_cross_term_fails_the_contract(shape, variant, A):
    """(1, (1, 1)) is left out: one weight per layer and logits that small keep every variant inside the contract."""
    weights, rows, _, p64, _ = _case(shape, A)
    ratio = float(ar.contract_ratio(br.forward(weights, rows, **br.VARIANTS[variant]), p64, True).max())
    print("MLP_ACTOR_BF16_WRONG %s A=%d %s contract=%.3f" % (mc.shape_id(shape), A, variant, ratio))
    assert ratio > 1.0


def _refused_call(lib, obs, action, a_prob, probs, A=16, ld=51, K=51, H1=256, H2=256, O=2, size=None, ptr=0x1000, mw=0, stream=None):
    """tests.test_mlp_actor.refused_call on the bf16x3 entry point."""
    import ctypes as C
    desc = _mlp(K, H1, H2, O, size, ptr)
    return lib.mdr_mlp_actor_sample_bf16x3(C.byref(desc), obs, ld, A, C.c_uint64(1), C.c_uint64(2), None, 0, mw, action, a_prob, probs, stream)


def test_the_export_and_its_signature():
    lib = nat.load()
    assert "mdr_mlp_actor_sample_bf16x3" in nat.EXPORTS
    assert lib.mdr_mlp_actor_sample_bf16x3.argtypes == lib.mdr_mlp_actor_sample.argtypes


def test_the_entry_point_refuses_what_the_fp32_one_refuses():
    lib = nat.load()
    p = 0x1000      # never dereferenced: every call below returns before a launch
    for kw, status in REFUSED:
        kw = dict(kw)
        obs, action = kw.pop("obs", p), kw.pop("action", p)
        assert _refused_call(lib, obs, action, p, p, **kw) == status, kw
    for kw in (dict(A=-1), dict(mw=-1), dict(ptr=None)):
        assert _refused_call(lib, p, p, p, p, **kw) == nat.MDR_ERR_INVALID, kw
    for kw in (dict(K=0), dict(H1=0), dict(H2=0)):
        assert _refused_call(lib, p, p, p, p, **kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert _refused_call(lib, p, p, None, None, A=0) == nat.MDR_OK      # no agents: nothing to launch


def test_precision_and_backend_strings():
    from mdr_amd.maddpg import DDPGNetworkMLP, GreedyDDPGActor
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import collect_maddpg_transitions
    actor = DDPGNetworkMLP(51, 2, 256)
    for bad in ("bf16", "auto", "", None):
        with pytest.raises(ValueError, match="precision"):
            FusedMLPActor(actor, precision=bad)
    with pytest.raises(ValueError, match="GPU"):      # a known precision: the module's own refusal, as before
        FusedMLPActor(actor, precision="bf16x3")
    with pytest.raises(ValueError, match="GPU"):
        collect_maddpg_transitions(None, actor, 1, actor_backend="hip-bf16x3")
    with pytest.raises(ValueError, match="GPU"):
        GreedyDDPGActor(actor, backend="hip-bf16x3")
    with pytest.raises(ValueError, match="fp32 only"):      # one net per agent has no bf16x3 form
        collect_maddpg_transitions(None, [actor, actor], 1, actor_backend="hip-bf16x3")
    with pytest.raises(ValueError, match="fp32 only"):
        GreedyDDPGActor([actor, actor], backend="hip-bf16x3")
    assert GreedyDDPGActor(actor).backend == "torch"
