"""The keyed forms of the banded TarMAC attention and of TarMAC-PPO's actor gradient (include/mdr_policy.h: mdr_tarmac_comm_keyed,
mdr_tarmac_comm_backward_keyed, mdr_tarmac_ppo_actor_grad_keyed): the Philox key of the dead-sender draw read from device memory.
A keyed call whose key holds the two words of a seed is the by-value call with that seed, bit for bit - forward output, dq, dk, dv;
flat gradient, loss and ratios -, with the step by value, from the device, or split between the two; another key gives other dead
senders and other results (the CPU restatement tests/tarmac_ref.py says beforehand that the masks differ); a NULL key is refused
with nothing written.  No tolerance anywhere: the by-value calls are held to fp64 by test_gpu_tarmac*.py and test_gpu_tarmac_ppo.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROB = 0.3
SEED, OTHER = 0x9E3779B97F4A7C15, 0x9E3779B97F4A7C16      # both words nonzero, the high one with its top bit set; one bit apart
STEP = 41

# (E, N, c, K, V)
SHAPES = [
    (13, 20, 10, 8, 16),      # the reference's sizes, the exact instantiation: 12 envs per workgroup plus a workgroup holding one
    (27, 20, 10, 8, 16),      # 540 agents: three workgroups, the last one partial
    (7, 5, 10, 16, 32),       # c clamped to N - 1, a non-exact instantiation
    (2, 300, 10, 8, 16),      # an env larger than a workgroup's tile: slices with halos (the by-value call takes it)
]


def _lib():
    import mdr_amd
    return mdr_amd.load_native()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _key_tensor(seed):
    from mdr_amd.graph_update import _i32
    return torch.tensor([_i32(seed & 0xFFFFFFFF), _i32(seed >> 32)], dtype=torch.int32, device=DEV)


def _inputs(shape):
    E, N, c, K, V = shape
    q, k, v = (torch.from_numpy(t.reshape(E * N, -1)).to(DEV) for t in tr.comm_inputs(E, N, K, V, seed=5))
    g = torch.from_numpy(np.random.default_rng([9, E, N]).standard_normal((E * N, V)).astype(np.float32)).to(DEV)
    return q, k, v, g


def _attention(shape, ops, mode, hop, step, step_dev, seed=None, key=None, fill=float("nan")):
    """Forward and backward, by value (``seed``) or keyed (``key``) -> (rc forward, rc backward, out, dq, dk, dv); the results start
    as ``fill``."""
    E, N, c, K, V = shape
    q, k, v, g = ops
    A = E * N
    lib = _lib()
    out = torch.full((A, V), fill, dtype=torch.float32, device=DEV)
    dq, dk, dv = (torch.full((A, d), fill, dtype=torch.float32, device=DEV) for d in (K, K, V))
    ws = torch.empty(max(int(lib.mdr_tarmac_comm_backward_workspace_bytes(A, K, V)), 16), dtype=torch.uint8, device=DEV)
    head = (_ptr(q), K, _ptr(k), K, _ptr(v), V, E, N, K, V, c, mode, C.c_float(PROB))
    tail_f = (C.c_uint64(step), _ptr(step_dev), hop, _ptr(out), V, _stream())
    if seed is not None:
        rc_f = lib.mdr_tarmac_comm(*head, C.c_uint64(seed), *tail_f)
    else:
        rc_f = lib.mdr_tarmac_comm_keyed(*head, _ptr(key), *tail_f)
    fwd = out if rc_f == 0 else torch.zeros_like(out)      # the backward of a refused forward: any finite `out` will do
    tail_b = (C.c_uint64(step), _ptr(step_dev), hop, _ptr(fwd), V, _ptr(g), V, _ptr(dq), K, _ptr(dk), K, _ptr(dv), V, _ptr(ws), _stream())
    if seed is not None:
        rc_b = lib.mdr_tarmac_comm_backward(*head, C.c_uint64(seed), *tail_b)
    else:
        rc_b = lib.mdr_tarmac_comm_backward_keyed(*head, _ptr(key), *tail_b)
    return rc_f, rc_b, out, dq, dk, dv


def test_the_exports_and_their_prototypes():
    lib = _lib()
    for name, by_value in (("mdr_tarmac_comm_keyed", "mdr_tarmac_comm"), ("mdr_tarmac_comm_backward_keyed", "mdr_tarmac_comm_backward")):
        assert name in nat.EXPORTS
        mine, theirs = getattr(lib, name).argtypes, getattr(lib, by_value).argtypes
        at = theirs.index(C.c_uint64)      # the seed: the first 64-bit unsigned argument
        assert list(mine) == list(theirs[:at]) + [C.c_void_p] + list(theirs[at + 1:])
    mine, theirs = lib.mdr_tarmac_ppo_actor_grad_keyed.argtypes, lib.mdr_tarmac_ppo_actor_grad.argtypes
    at = theirs.index(C.c_uint64)
    assert list(mine) == list(theirs[:at]) + [C.c_void_p, C.c_uint64, C.c_void_p] + list(theirs[at + 2:])      # key, step, step_dev
    assert "mdr_tarmac_ppo_actor_grad_keyed" in nat.EXPORTS


@pytest.mark.parametrize("hop", [0, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_keyed_attention_is_the_by_value_call(shape, hop):
    E, N, c, K, V = shape
    # the restatement first: the two keys silence different senders at this shape, step and hop, and some sender is heard at all
    mask, other = (tr.dead_mask(E, N, PROB, s, STEP, hop=hop) for s in (SEED, OTHER))
    assert tr.clamp(c, N) >= 1 and (mask != other).any() and mask.any() and not mask.all()
    ops = _inputs(shape)
    ref = _attention(shape, ops, tr.NEIGHBOURS, hop, STEP, None, seed=SEED)
    assert ref[:2] == (0, 0) and all(bool(torch.isfinite(t).all()) for t in ref[2:])
    key = _key_tensor(SEED)
    cursor = torch.tensor([STEP - 4], dtype=torch.int32, device=DEV)
    for step, step_dev in ((STEP, None), (4, cursor)):      # the step by value; split between the argument and device memory
        got = _attention(shape, ops, tr.NEIGHBOURS, hop, step, step_dev, key=key)
        assert got[:2] == (0, 0)
        for name, a, b in zip(("out", "dq", "dk", "dv"), ref[2:], got[2:]):
            assert torch.equal(a, b), (name, step)
    # the key is read when the kernel runs: other words in the same tensor, other dead senders, other results
    key.copy_(_key_tensor(OTHER))
    moved = _attention(shape, ops, tr.NEIGHBOURS, hop, STEP, None, key=key)
    assert moved[:2] == (0, 0)
    for name, a, b in zip(("out", "dq", "dk", "dv"), ref[2:], moved[2:]):
        assert not torch.equal(a, b), name
    theirs = _attention(shape, ops, tr.NEIGHBOURS, hop, STEP, None, seed=OTHER)
    for a, b in zip(theirs[2:], moved[2:]):
        assert torch.equal(a, b)


def test_keyed_attention_in_mode_none():
    shape = SHAPES[0]
    ops = _inputs(shape)
    ref = _attention(shape, ops, tr.NONE, 0, STEP, None, seed=SEED)
    got = _attention(shape, ops, tr.NONE, 0, STEP, None, key=_key_tensor(SEED))
    assert ref[:2] == got[:2] == (0, 0)
    for a, b in zip(ref[2:], got[2:]):
        assert torch.equal(a, b) and not bool(a.any())      # the constant zero and its gradients


@pytest.mark.parametrize("mode", [tr.NEIGHBOURS, tr.NONE])
def test_a_null_key_is_refused_with_nothing_written(mode):
    shape = SHAPES[2]
    rc_f, rc_b, *results = _attention(shape, _inputs(shape), mode, 0, STEP, None, key=None, fill=7.0)
    assert rc_f == rc_b == nat.MDR_ERR_INVALID
    torch.cuda.synchronize()
    for t in results:
        assert bool((t == 7.0).all())


# -- mdr_tarmac_ppo_actor_grad_keyed ---------------------------------------------------------------------------------------------------
M, N, F, H, K, V = 12, 5, 22, 16, 8, 16


def _actor_case():
    from mdr_amd.tarmac import TarMACActor
    torch.manual_seed(21)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=2, comm_defect_prob=0.25).to(DEV)
    gen = torch.Generator().manual_seed(22)
    state = torch.randn((M, N, F), generator=gen).to(DEV)
    action = torch.randint(0, 2, (M, N), generator=gen).to(DEV)
    old_prob = (0.25 + 0.5 * torch.rand((M, N), generator=gen)).to(DEV)
    index = torch.randperm(M, generator=gen)[:7].to(DEV)
    adv = torch.randn((7, N), generator=gen).to(DEV)
    return actor, state, action, old_prob, index, adv


def _actor_grad(case, fill=float("nan"), **how):
    """One call on buffers of its own -> (flat gradient, loss, ratios)."""
    from mdr_amd import _learner as L
    from mdr_amd import tarmac_ppo as tp
    actor, state, action, old_prob, index, adv = case
    desc = tp._desc(actor)
    floats, nbytes = tp._actor_sizes(desc, 7, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    flat = torch.full((floats,), fill, dtype=torch.float32, device=DEV)
    loss = torch.full((), fill, dtype=torch.float32, device=DEV)
    ratio = torch.full((7, N), fill, dtype=torch.float32, device=DEV)
    tp._actor_launch(desc, state, F, action, old_prob, index, 7, N, adv, ws, flat, loss, ratio, L.stream(torch.device(DEV)), 0.2, **how)
    return flat, loss, ratio


def test_keyed_actor_gradient_is_the_by_value_call():
    case = _actor_case()
    # 7 env-steps of 5 agents, 2 senders each: the two keys silence different senders of the minibatch
    mask, other = (tr.dead_mask(7, N, 0.25, s, STEP) for s in (SEED, OTHER))
    assert (mask != other).any() and mask.any()
    ref = _actor_grad(case, seed=SEED, step=STEP)
    assert all(bool(torch.isfinite(t).all()) for t in ref) and bool(ref[0].any())
    key = _key_tensor(SEED)
    cursor = torch.tensor([STEP - 3], dtype=torch.int32, device=DEV)
    for how in (dict(step=STEP), dict(step=3, step_dev=cursor)):
        got = _actor_grad(case, key=key, **how)
        for name, a, b in zip(("grad", "loss", "ratio"), ref, got):
            assert torch.equal(a, b), (name, sorted(how))
    moved = _actor_grad(case, key=_key_tensor(OTHER), step=STEP)
    theirs = _actor_grad(case, seed=OTHER, step=STEP)
    for name, a, b, c in zip(("grad", "loss", "ratio"), ref, moved, theirs):
        assert not torch.equal(a, b) and torch.equal(b, c), name
    with pytest.raises(ValueError, match="step_dev goes with key"):
        _actor_grad(case, seed=SEED, step=3, step_dev=cursor)


def test_keyed_actor_gradient_refuses_a_null_key():
    from mdr_amd import _learner as L
    from mdr_amd import tarmac_ppo as tp
    actor, state, action, old_prob, index, adv = _actor_case()
    desc = tp._desc(actor)
    floats, nbytes = tp._actor_sizes(desc, 7, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    flat = torch.full((floats,), 7.0, dtype=torch.float32, device=DEV)
    loss = torch.full((), 7.0, dtype=torch.float32, device=DEV)
    rc = _lib().mdr_tarmac_ppo_actor_grad_keyed(C.byref(desc), _ptr(state), F, _ptr(index), 7, N, _ptr(action), _ptr(old_prob), _ptr(adv),
                                                C.c_float(0.2), None, C.c_uint64(STEP), None, 0, _ptr(ws), _ptr(flat), _ptr(loss), None,
                                                L.stream(torch.device(DEV)))
    assert rc == nat.MDR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all()) and float(loss) == 7.0
