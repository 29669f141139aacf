"""Observe -> act for the 256-unit fused actor, what needs no device: the binding of mdr_env_mlp_actor_sample[_bf16x3], the host-side
refusals of FusedMLPActor.sample_env / observe_supported and of GreedyDDPGActor.sample_env, and the new keywords of the loops (the GPU
side: tests/test_gpu_mlp_actor_observe.py)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mdr_env_mlp_actor_sample", "mdr_env_mlp_actor_sample_bf16x3")


def _prototype(name):
    header = open(os.path.join(ROOT, "include", "mdr_policy.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, "%s is not declared in include/mdr_policy.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_are_in_the_header_the_binding_and_the_integration_table(name):
    from mdr_amd import _native as nat
    args = _prototype(name)
    assert [a.split()[-1].lstrip("*") for a in args] == ["env", "spec", "actor", "seed", "step", "step_dev", "greedy", "max_workgroups", "action",
                                                         "a_prob", "probs", "rows_out", "stream"]
    assert name in nat.EXPORTS
    lib = nat.load()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) == 13
    assert fn.argtypes[1] is C.POINTER(nat.MdrObsSpec) and fn.argtypes[2] is C.POINTER(nat.MdrMlp)
    assert fn.argtypes[3] is C.c_uint64 and fn.argtypes[4] is C.c_uint64
    assert nat.MDR_ABI_VERSION == 5 == lib.mdr_abi_version()      # new functions under the same ABI: nothing existing changed
    assert fn(None, None, None, 0, 0, None, 0, 0, None, None, None, None, None) == nat.MDR_ERR_INVALID
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


class _Env:
    """What sample_env looks at before it touches the device."""

    def __init__(self, N=20, sharded=False, **spec):
        from mdr_amd import _native as nat
        self.nb_envs, self.nb_houses, self.sharded, self.device = 3, N, sharded, torch.device("cuda:0")
        self.steps_taken = 0
        self._spec = nat.MdrObsSpec()
        self._spec.nb_comm = 10
        for k, v in spec.items():
            setattr(self._spec, k, v)

    def _obs_spec(self, layout):
        assert layout == "rows"
        return self._spec


def _net(F=51, H=256):
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(0)
    return DDPGNetworkMLP(F, 2, H)


def _fused(F=51, precision="fp32"):
    """A FusedMLPActor around a net on the host, as the constructor would not make it: every check below comes before any launch."""
    from mdr_amd.mlp_actor import FusedMLPActor
    fused = FusedMLPActor.__new__(FusedMLPActor)
    fused.module, fused.greedy, fused.precision, fused._lib = _net(F), False, precision, None
    return fused


REFUSED = [dict(state_hour=1), dict(state_day=1), dict(state_solar_gain=1), dict(state_thermal=1), dict(state_hvac=1),
           dict(message_thermal=1), dict(message_hvac=1), dict(nb_comm=6), dict(random_links=1), dict(comm_defect_prob=0.1),
           dict(sharded=True), dict(N=10)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(sorted(kw)))
def test_envs_outside_the_default_observation_are_refused_on_the_host(kw, precision):
    from mdr_amd.mlp_actor import default_observation_refusal
    fused = _fused(precision=precision)
    env = _Env(**kw)
    assert default_observation_refusal(env) is not None and not fused.observe_supported(env)
    with pytest.raises(ValueError, match=r"FusedMLPActor\.sample_env: "):
        fused.sample_env(env, 0, 0)


def test_the_actor_side():
    from mdr_amd.mlp_actor import FusedMLPActors, default_observation_refusal
    for N in (11, 20, 32, 1024):
        assert default_observation_refusal(_Env(N=N)) is None
    for F in (47, 64):
        narrow = _fused(F)
        assert not narrow.observe_supported(_Env())
        with pytest.raises(ValueError, match="51"):
            narrow.sample_env(_Env(), 0, 0)
    with pytest.raises(ValueError, match="GPU"):      # a covered env, but the parameters are on the host: still before any launch
        _fused().sample_env(_Env(), 0, 0)
    assert not _fused().observe_supported(_Env())
    assert not hasattr(FusedMLPActors, "sample_env") and not hasattr(FusedMLPActors, "observe_supported")      # one net per agent: rows


def test_greedy_ddpg_actor_serves_one_shared_hip_net_only():
    from mdr_amd.maddpg import GreedyDDPGActor
    by_torch = GreedyDDPGActor(_net())
    assert not by_torch.observe_supported(_Env())
    with pytest.raises(ValueError, match="sample_env"):
        by_torch.sample_env(_Env())
    per_agent = GreedyDDPGActor([_net(), _net()])
    assert not per_agent.observe_supported(_Env())
    with pytest.raises(ValueError, match="sample_env"):
        per_agent.sample_env(_Env())
    params = list(inspect.signature(GreedyDDPGActor.sample_env).parameters)
    assert params == ["self", "env", "seed", "step", "action", "step_dev"]
    # a hip actor is refused before any launch where its FusedMLPActor is
    hip = GreedyDDPGActor(_net())
    hip.backend, hip._fused = "hip", _fused()
    assert not hip.observe_supported(_Env(nb_comm=6)) and not hip.observe_supported(_Env())
    with pytest.raises(ValueError, match="sample_env"):
        hip.sample_env(_Env(nb_comm=6))
    with pytest.raises(ValueError, match="GPU"):
        hip.sample_env(_Env())


def test_keywords_are_last_and_resolve_on_the_host():
    from mdr_amd.maddpg import GreedyDDPGActor, train_maddpg
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import _mlp_observe_act, collect_maddpg_transitions, deploy_policy
    for fn in (collect_maddpg_transitions, train_maddpg):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "observe_act" and params[-1].default is False
        assert params[-2].name == "actor_backend" and params[-2].default == "torch"
    params = list(inspect.signature(deploy_policy).parameters.values())
    assert [p.name for p in params] == ["env", "policy", "nb_steps", "seed", "use_graph", "policy_precision", "greedy", "observe_act"]
    assert params[-1].default is None
    sig = inspect.signature(FusedMLPActor.sample_env)
    assert list(sig.parameters) == ["self", "env", "seed", "step", "step_dev", "greedy", "action", "a_prob", "want_probs", "rows_out",
                                    "max_workgroups"]
    assert [sig.parameters[k].default for k in ("step_dev", "greedy", "action", "a_prob", "want_probs", "rows_out", "max_workgroups")] == \
        [None, None, None, None, False, None, 0]
    # opt-in: None and False keep the rows, whatever the policy; True must be servable
    by_torch, fused = GreedyDDPGActor(_net()), _fused()
    for policy in (by_torch, fused, object()):
        assert _mlp_observe_act(_Env(), policy, None) is False and _mlp_observe_act(_Env(), policy, False) is False
    assert _mlp_observe_act(_Env(), object(), True) is False      # not this function's policy: the TarMAC resolution decides
    for env, policy in ((_Env(), by_torch), (_Env(), GreedyDDPGActor([_net(), _net()])), (_Env(nb_comm=6), fused), (_Env(), fused)):
        with pytest.raises(ValueError, match="observe_act"):
            _mlp_observe_act(env, policy, True)
    # the collection refuses before it touches the env
    for actor, backend in ((_net(), "torch"), ([_net(), _net()], "torch")):
        env = _Env()
        with pytest.raises(ValueError, match="observe_act"):
            collect_maddpg_transitions(env, actor, 2, actor_backend=backend, observe_act=True)
        assert env.steps_taken == 0
