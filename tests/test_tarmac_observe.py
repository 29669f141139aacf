"""Observe -> act for the fused TarMAC actor, what needs no device: the binding of mdr_env_tarmac_actor_sample, the argument checks
of FusedTarMACActor.sample_env / observe_supported, and the normStateDict-to-window position map (the GPU side:
tests/test_gpu_tarmac_observe.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype(name):
    header = open(os.path.join(ROOT, "include", "mdr_policy.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, "%s is not declared in include/mdr_policy.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_point_is_in_the_header_the_binding_and_the_integration_table():
    from mdr_amd import _native as nat
    args = _prototype("mdr_env_tarmac_actor_sample")
    assert [a.split()[-1].lstrip("*") for a in args] == ["env", "spec", "actor", "seed", "step", "step_dev", "workspace", "action", "a_prob",
                                                         "probs", "rows_out", "stream"]
    assert "mdr_env_tarmac_actor_sample" in nat.EXPORTS
    lib = nat.load()
    fn = lib.mdr_env_tarmac_actor_sample
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) == 12
    # the rows entry point plus env, spec and rows_out instead of obs and the two sizes
    assert len(lib.mdr_tarmac_actor_sample.argtypes) == len(_prototype("mdr_tarmac_actor_sample")) == 12
    assert fn.argtypes[1] is C.POINTER(nat.MdrObsSpec) and fn.argtypes[3] is C.c_uint64 and fn.argtypes[4] is C.c_uint64
    assert lib.mdr_abi_version() == nat.MDR_ABI_VERSION      # a new function under the same ABI: nothing existing changed
    assert fn(None, None, None, 0, 0, None, None, None, None, None, None, None) == nat.MDR_ERR_INVALID
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`mdr_env_tarmac_actor_sample`" in table


class _Env:
    """What sample_env looks at before it touches the device."""

    def __init__(self, N=20, sharded=False, **spec):
        from mdr_amd import _native as nat
        self.nb_envs, self.nb_houses, self.sharded, self.device = 3, N, sharded, torch.device("cuda:0")
        self._spec = nat.MdrObsSpec()
        self._spec.nb_comm = 10
        for k, v in spec.items():
            setattr(self._spec, k, v)

    def _obs_spec(self, layout):
        assert layout == "rows"
        return self._spec


def _fused(F=51, **kw):
    from mdr_amd.tarmac import FusedTarMACActor, TarMACActor
    torch.manual_seed(0)
    return FusedTarMACActor(TarMACActor(F, **kw))


REFUSED = [dict(state_hour=1), dict(state_day=1), dict(state_solar_gain=1), dict(state_thermal=1), dict(state_hvac=1),
           dict(message_thermal=1), dict(message_hvac=1), dict(nb_comm=6), dict(nb_comm=9, N=10), dict(random_links=1),
           dict(comm_defect_prob=0.1), dict(sharded=True), dict(N=10)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(sorted(kw)))
def test_envs_outside_the_default_observation_are_refused_on_the_host(kw):
    fused = _fused()
    env = _Env(**kw)
    assert not fused.observe_supported(env)
    with pytest.raises(ValueError, match="sample_env"):
        fused.sample_env(env, 0, 0)


def test_supported_envs_and_the_actor_side():
    # the actor's own attention settings are not the env's message senders
    for kw in (dict(), dict(number_agents_comm=4), dict(comm_mode="none"), dict(comm_defect_prob=0.5), dict(num_hops=3), dict(with_comm=False),
               dict(hidden_state_size=32, num_key=4, num_value=8)):
        fused = _fused(**kw)
        assert fused.observe_supported(_Env()) and fused.observe_supported(_Env(N=11)) and fused.observe_supported(_Env(N=1024))
    for F in (47, 52, 64):
        narrow = _fused(F)
        assert not narrow.observe_supported(_Env())
        with pytest.raises(ValueError, match="51"):
            narrow.sample_env(_Env(), 0, 0)
    with pytest.raises(ValueError, match="GPU"):      # a covered env, but the parameters are on the host: still before any launch
        _fused().sample_env(_Env(), 0, 0)


def test_rollout_keyword_is_last_and_resolves_on_the_host():
    import inspect

    from mdr_amd.rollout import _tarmac_observe_act, collect_tarmac_rollout, deploy_policy
    from mdr_amd.tarmac import TarMACActor
    for fn in (collect_tarmac_rollout, deploy_policy):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "observe_act" and params[-1].default is None
    fused = _fused()
    assert _tarmac_observe_act(_Env(), fused, None) is True and _tarmac_observe_act(_Env(), fused, True) is True
    assert _tarmac_observe_act(_Env(), fused, False) is False
    assert _tarmac_observe_act(_Env(nb_comm=6), fused, None) is False and _tarmac_observe_act(_Env(), TarMACActor(51), None) is False
    for env, policy in ((_Env(nb_comm=6), fused), (_Env(), TarMACActor(51)), (_Env(), _fused(47))):
        with pytest.raises(ValueError, match="observe_act"):
            _tarmac_observe_act(env, policy, True)


def test_window_positions_invert_the_observe_feature_order():
    """FEATURES_OBSERVE: staged float k holds normStateDict index (k < 40 ? 11 + k : k - 40) (policy.observe_feature_order); the
    TarMAC forms read normStateDict index n at float (n < 11 ? 40 + n : n - 11)."""
    from mdr_amd.policy import OBSERVE_NUM_STATE, observe_feature_order
    from mdr_amd.tarmac import observe_window_positions
    pos = observe_window_positions()
    n = np.arange(OBSERVE_NUM_STATE)
    assert OBSERVE_NUM_STATE == 51 and pos.shape == (51,)
    assert np.array_equal(pos, np.where(n < 11, 40 + n, n - 11))
    assert np.array_equal(observe_feature_order()[pos], n) and np.array_equal(np.sort(pos), n)
    # the k-step orders of the two precisions cover every feature once and pad only past it
    fp32 = np.array([13 * g + s for g in range(4) for s in range(13)])
    bf16 = np.array([32 * s + 8 * g + j for s in range(2) for g in range(4) for j in range(8)])
    assert np.array_equal(np.sort(fp32), np.arange(52)) and np.array_equal(np.sort(bf16), np.arange(64))
