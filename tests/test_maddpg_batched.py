"""The batched form of MADDPG's unshared update without a GPU: the exports and their ctypes signatures, what the entry points refuse
on the host (fake non-NULL pointers that are never dereferenced: every call below returns before a launch, as
tests/test_mlp_actor_bf16.py::_refused_call does it), and the ``ValueError``s of ``MADDPGLearner(agent_steps="batched")`` and
``optim.step_nets``."""
import ctypes as C

import pytest
import torch

from mdr_amd import _native as nat

P = 0x1000      # a fake device pointer
N, F_LEN, H, B = 3, 5, 20, 16
ALL = ("mdr_maddpg_workspace_bytes_all", "mdr_maddpg_target_all", "mdr_maddpg_critic_grad_all", "mdr_maddpg_actor_grad_all")
ADAM = ("mdr_adam_nets_table_bytes", "mdr_adam_nets_bind", "mdr_adam_step_nets")


def _desc(K, H1=H, H2=H, O=2, size=None, ptr=P):
    size = C.sizeof(nat.MdrMlp) if size is None else size
    return nat.MdrMlp(size, K, H1, H2, O, *([ptr] * 6))


def _nets(n=N, actor=None, critic=None, **kw):
    """(host array of n actors, of n critics); ``actor`` / ``critic``: {agent: keyword arguments of _desc} for single nets."""
    actor, critic = actor or {}, critic or {}
    actors = (nat.MdrMlp * max(n, 1))(*[_desc(**dict(dict(K=F_LEN, O=2), **actor.get(k, {}))) for k in range(max(n, 1))])
    critics = (nat.MdrMlp * max(n, 1))(*[_desc(**dict(dict(K=N * (F_LEN + 2), O=1), **critic.get(k, {}))) for k in range(max(n, 1))])
    return actors, critics


def _target(lib, n=N, rows=B, index=P, y=P, mw=0, tau=1.0, **kw):
    actors, critics = _nets(n, **kw)
    return lib.mdr_maddpg_target_all(actors, critics, P, N * F_LEN, P, index, rows, n, P, C.c_float(tau), C.c_float(0.99), mw, y, None, P, None)


def _critic(lib, n=N, rows=B, index=P, y=P, mw=0, ws=P, tau=None, **kw):
    _, critics = _nets(n, **kw)
    return lib.mdr_maddpg_critic_grad_all(critics, P, N * F_LEN, P, index, rows, n, y, mw, ws, P, P, None, None)


def _actor(lib, n=N, rows=B, index=P, y=P, mw=0, ws=P, tau=1.0, **kw):
    actors, critics = _nets(n, **kw)
    return lib.mdr_maddpg_actor_grad_all(actors, critics, P, N * F_LEN, P, index, rows, n, y, C.c_float(tau), C.c_float(1e-3), mw, ws, P, P, None,
                                         None, None)


CALLS = (_target, _critic, _actor)


def test_the_exports_and_their_signatures():
    lib = nat.load()
    for name in ALL + ADAM:
        assert name in nat.EXPORTS and hasattr(lib, name), name
    mlp, vp, i32, i64, f = C.POINTER(nat.MdrMlp), C.c_void_p, C.c_int32, C.c_int64, C.c_float
    # the single-agent signatures without `agent` (and, for the target, without nb_nets and with an array of critics)
    single = list(lib.mdr_maddpg_target_agents.argtypes)
    assert lib.mdr_maddpg_target_all.argtypes == [mlp, mlp, vp, i64, vp, vp, i64, i32, vp, f, f, i32, vp, vp, vp, vp]
    assert lib.mdr_maddpg_target_all.argtypes == [single[0]] + single[2:9] + single[10:]
    single = list(lib.mdr_maddpg_critic_grad.argtypes)
    assert lib.mdr_maddpg_critic_grad_all.argtypes == single == [mlp, vp, i64, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp]
    single = list(lib.mdr_maddpg_actor_grad.argtypes)
    assert lib.mdr_maddpg_actor_grad_all.argtypes == single[:8] + single[9:]
    assert lib.mdr_maddpg_workspace_bytes_all.argtypes == lib.mdr_maddpg_workspace_bytes.argtypes
    assert lib.mdr_maddpg_workspace_bytes_all.restype == i64 and lib.mdr_adam_nets_table_bytes.restype == i64
    assert lib.mdr_adam_nets_bind.argtypes == [vp, i32, C.POINTER(nat.MdrAdamSegments), vp, vp, vp]
    d = C.c_double
    assert lib.mdr_adam_step_nets.argtypes == [vp, i32, i64, d, d, d, d, i64, d, d, d, vp, vp, vp]


def test_the_workspace_is_the_single_calls_times_the_agents():
    lib = nat.load()
    actors, critics = _nets()
    for rows in (0, 1, 16, 17, 64):
        one = lib.mdr_maddpg_workspace_bytes(C.byref(actors[0]), C.byref(critics[0]), N, rows, 0)
        assert lib.mdr_maddpg_workspace_bytes_all(C.byref(actors[0]), C.byref(critics[0]), N, rows, 0) == max(N * one if rows else 16, 16)
    assert lib.mdr_maddpg_workspace_bytes_all(C.byref(actors[0]), C.byref(critics[0]), N, -1, 0) == -1
    assert lib.mdr_maddpg_workspace_bytes_all(None, C.byref(critics[0]), N, 16, 0) == -1
    wide = _desc(K=33 * (F_LEN + 2), O=1)
    assert lib.mdr_maddpg_workspace_bytes_all(C.byref(actors[0]), C.byref(wide), 33, 16, 0) == -1


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.__name__.strip("_"))
def test_the_entry_points_refuse_on_the_host(call):
    lib = nat.load()
    inv, uns = nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED
    assert call(lib, index=None) == inv and call(lib, y=None) == inv      # NULL arguments (y: the target's noise, the actor's noise)
    assert call(lib, critic={1: dict(ptr=None)}) == inv                  # a NULL weight pointer in one net
    assert call(lib, critic={2: dict(size=8)}) == inv                    # a struct_size that is not the header's
    assert call(lib, n=0) == inv and call(lib, n=-1) == inv
    assert call(lib, n=33) == uns                                        # more nets than the table holds
    assert call(lib, critic={1: dict(H1=H + 1)}) == uns                  # nets of differing shapes
    assert call(lib, critic={k: dict(K=N * (F_LEN + 2) + 1) for k in range(N)}) == inv      # num_state != N (F + 2)
    assert call(lib, critic={k: dict(H1=257) for k in range(N)}) == uns  # a shape outside the limits
    assert call(lib, rows=-1) == inv and call(lib, mw=-1) == inv
    if call is not _critic:
        assert call(lib, tau=0.0) == inv and call(lib, tau=float("nan")) == inv
        assert call(lib, actor={1: dict(H2=H - 1)}) == uns
        assert call(lib, actor={k: dict(K=F_LEN + 1) for k in range(N)}) == inv
        assert call(lib, actor={0: dict(size=0)}) == inv
    if call is not _target:
        assert call(lib, ws=None) == inv and call(lib, ws=P + 4) == inv      # a missing and a misaligned workspace
    else:
        assert call(lib, rows=0) == nat.MDR_OK      # no rows: nothing to launch, as mdr_maddpg_target


def test_the_optimiser_entry_points_refuse_on_the_host():
    lib = nat.load()
    inv, uns = nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED
    assert lib.mdr_adam_nets_table_bytes(-1) == -1 and lib.mdr_adam_nets_table_bytes(0) == 0
    one = lib.mdr_adam_nets_table_bytes(1)
    assert one > 0 and one % 16 == 0 and lib.mdr_adam_nets_table_bytes(20) == 20 * one
    seg = nat.MdrAdamSegments()
    seg.struct_size, seg.nb_segments = C.sizeof(nat.MdrAdamSegments), 1
    seg.seg[0].param, seg.seg[0].grad, seg.seg[0].count = P, P, 10
    assert lib.mdr_adam_nets_bind(None, 0, C.byref(seg), P, P, None) == inv
    assert lib.mdr_adam_nets_bind(P + 4, 0, C.byref(seg), P, P, None) == inv
    assert lib.mdr_adam_nets_bind(P, -1, C.byref(seg), P, P, None) == inv
    assert lib.mdr_adam_nets_bind(P, 0, None, P, P, None) == inv
    assert lib.mdr_adam_nets_bind(P, 0, C.byref(seg), None, P, None) == inv
    seg.nb_segments = 33
    assert lib.mdr_adam_nets_bind(P, 0, C.byref(seg), P, P, None) == uns
    seg.nb_segments, seg.struct_size = 1, 8
    assert lib.mdr_adam_nets_bind(P, 0, C.byref(seg), P, P, None) == inv
    seg.struct_size, seg.seg[0].param = C.sizeof(nat.MdrAdamSegments), None
    assert lib.mdr_adam_nets_bind(P, 0, C.byref(seg), P, P, None) == inv

    def step(table=P, n=2, floats=100, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1, clip=0.5, clamp=float("inf"), tau=0.0, ws=P, norm=None):
        return lib.mdr_adam_step_nets(table, n, floats, lr, b1, b2, eps, t, clip, clamp, tau, ws, norm, None)

    for kw in (dict(table=None), dict(n=-1), dict(floats=-1), dict(t=0), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0),
               dict(tau=1.5), dict(clamp=0.0), dict(ws=None), dict(ws=P + 4)):
        assert step(**kw) == inv, kw
    assert step(n=0) == nat.MDR_OK      # no nets: nothing to launch


def test_the_learner_refuses_what_the_batched_form_does_not_cover():
    from mdr_amd.maddpg import DDPGNetworkMLP, MADDPGLearner
    from mdr_amd.optim import FusedAdam
    actors = [DDPGNetworkMLP(F_LEN, 2, H) for _ in range(N)]
    critics = [DDPGNetworkMLP(N * (F_LEN + 2), 1, H) for _ in range(N)]
    good = dict(shared=False, backend="hip", optimizer=FusedAdam, agent_steps="batched")
    for kw, word in ((dict(shared=True), "shared=False"), (dict(backend="torch"), "backend='hip'"), (dict(backend="auto"), "backend='hip'"),
                     (dict(optimizer=torch.optim.Adam), "FusedAdam"), (dict(graph=True), "graph=False")):
        with pytest.raises(ValueError, match=word):
            MADDPGLearner(actors, critics, N, 1e-3, 1e-3, **dict(good, **kw))
    with pytest.raises(ValueError, match="agent_steps"):
        MADDPGLearner(actors, critics, N, 1e-3, 1e-3, **dict(good, agent_steps="parallel"))
    with pytest.raises(ValueError, match="agent_steps"):
        MADDPGLearner.from_config(dict(lr_actor=1e-3, lr_critic=1e-3, gamma=0.99, soft_tau=0.01, gumbel_softmax_tau=1.0, batch_size=B,
                                       buffer_capacity=64, DDPG_shared=False), actors, critics, N, backend="hip", optimizer=FusedAdam,
                                  agent_steps="parallel")
    # the default is today's loop, and it still builds on the CPU with the torch backend
    assert MADDPGLearner(actors, critics, N, 1e-3, 1e-3, shared=False, backend="torch", buffer_capacity=64).agent_steps == "sequential"


def test_step_nets_refuses_optimisers_that_do_not_go_together():
    from mdr_amd import optim
    assert optim.nets_refusal([]) == "no optimisers"
    assert "FusedAdam" in optim.nets_refusal([torch.optim.Adam([torch.zeros(1, requires_grad=True)])])
    with pytest.raises(ValueError, match="step_nets"):
        optim.step_nets([])
