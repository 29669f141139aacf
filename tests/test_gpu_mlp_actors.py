"""mdr_mlp_actors_sample (csrc/mdr_mlp_actor.hip, the per-net forms) through FusedMLPActors: one actor per agent, row e N + k through net
k.  The draw is keyed by the row's index in the whole batch, so the shared kernel is an exact oracle: rows k::N of every output are,
bit for bit, what mdr_mlp_actor_sample(net k) gives those rows when it runs on the WHOLE batch.  Independent of the old kernel, one
case is held against the fp64 forward and the restated Philox draw by tests/test_gpu_mlp_actor.py's own rule (check_outputs).  Then
what the header promises beside the numbers: the same bits whatever the grid (one workgroup walks every net and reloads the weights N
times), a row stride beyond F, the device-side step, greedy, weights read in place, refused calls that write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import actor_ref as ar
from tests import mlp_actor_cases as mc
from tests.test_gpu_actor_forms import check_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, STEP = 9, 3
SHAPES = [mc.SHAPES[0], mc.SHAPES[3], mc.SHAPES[4], mc.SHAPES[6], mc.SHAPES[7]]      # (65, ...) takes the form of F > 64
NETS = (1, 2, 3, 20)
ENVS = (1, 33)      # a partial tile of 32 envs; a second tile


def make_actors(shape, N, equal=False):
    """N ActorMLPs of a shape on the device: net k is mlp_actor_cases' net with the seed moved by k (all the same one with `equal`)."""
    return [ar.make_actor(shape[0], shape[1], seed=mc.NET_SEED + (0 if equal else 101 * k), scale=mc.NET_SCALE, keep=mc.NET_KEEP).to(DEV)
            for k in range(N)]


def _fused(actors, greedy=False):
    from mdr_amd.mlp_actor import FusedMLPActors
    return FusedMLPActors(actors, greedy=greedy)


def _shared(actor, rows, **kw):
    from mdr_amd.mlp_actor import FusedMLPActor
    return FusedMLPActor(actor).sample(rows, SEED, STEP, want_probs=True, **kw)


def _same(got, want):
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("N", NETS)
@pytest.mark.parametrize("shape", SHAPES, ids=mc.shape_id)
def test_every_agents_rows_have_the_bits_of_the_shared_kernel_on_its_own_net(shape, N, E):
    actors = make_actors(shape, N)
    rows = mc.rows(shape, E * N).to(DEV)
    got = _fused(actors).sample(rows, SEED, STEP, want_probs=True)
    g_got = _fused(actors, greedy=True).sample(rows, SEED, STEP, want_probs=True)
    assert bool(torch.isfinite(got[2]).all())
    for k in range(N):
        want = _shared(actors[k], rows)
        _same([x[k::N] for x in got], [x[k::N] for x in want])
        _same([x[k::N] for x in g_got], [x[k::N] for x in _shared(actors[k], rows, greedy=True)])
    if N > 1 and shape[0] > 1:      # the nets do differ: a kernel that served every row by net 0 fails above
        assert not torch.equal(_shared(actors[0], rows)[2][1::N], _shared(actors[1], rows)[2][1::N])


def test_against_fp64_and_the_restated_draw():
    shape, N, E = mc.SHAPES[0], 3, 33
    actors = make_actors(shape, N)
    rows = mc.rows(shape, E * N).to(DEV)
    action, a_prob, probs = _fused(actors).sample(rows, SEED, STEP, want_probs=True)
    g_action, _ = _fused(actors).sample(rows, SEED, STEP, greedy=True)
    for k in range(N):
        agents = np.arange(E, dtype=np.uint64) * N + k
        picked = [t[k::N].contiguous().cpu().numpy() for t in (rows, action, a_prob, probs, g_action)]
        check_outputs("mlp_actors %s net %d" % (mc.shape_id(shape), k), 0, ar.module_weights(actors[k]), *picked, SEED, STEP,
                      agents=agents, cap=False)      # 33 rows: a share of them means nothing


@pytest.mark.parametrize("shape", [mc.SHAPES[0], mc.SHAPES[3]], ids=mc.shape_id)
def test_equal_nets_give_the_shared_kernels_bits(shape):
    N, E = 3, 33
    actors = make_actors(shape, N, equal=True)
    rows = mc.rows(shape, E * N).to(DEV)
    _same(_fused(actors).sample(rows, SEED, STEP, want_probs=True), _shared(actors[0], rows))


@pytest.mark.parametrize("shape", [mc.SHAPES[0], mc.SHAPES[3]], ids=mc.shape_id)
def test_the_grid_does_not_change_a_bit(shape):
    N, E = 20, 70      # three tiles per net, the last partial; with one workgroup the weights are loaded 20 times
    fused = _fused(make_actors(shape, N))
    rows = mc.rows(shape, E * N).to(DEV)
    outs = [fused.sample(rows, SEED, STEP, want_probs=True, max_workgroups=mw) for mw in (1, 2, 0)]
    for other in outs[1:]:
        _same(outs[0], other)
    assert bool(torch.isfinite(outs[0][2]).all())


def test_a_row_stride_beyond_f_and_canaries_around_the_outputs():
    shape, N, E = mc.SHAPES[0], 3, 33
    F, A = shape[0], N * E
    fused = _fused(make_actors(shape, N))
    rows = mc.rows(shape, A).to(DEV)
    want = fused.sample(rows, SEED, STEP, want_probs=True)
    wide = torch.full((A, F + 5), float("nan"), device=DEV)
    wide[:, :F] = rows
    _same(fused.sample(wide[:, :F], SEED, STEP, want_probs=True), want)
    act = torch.full((A + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    prob = torch.full((A + 64,), float("nan"), device=DEV)
    got = fused.sample(wide[:, :F], SEED, STEP, action=act[32:32 + A], a_prob=prob[32:32 + A])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((act[:32] == 0xEE).all()) and bool((act[32 + A:] == 0xEE).all())
    assert bool(prob[:32].isnan().all()) and bool(prob[32 + A:].isnan().all())


def test_the_device_side_step_and_the_draws_counter():
    shape, N, E = mc.SHAPES[0], 3, 33
    A = N * E
    fused = _fused(make_actors(shape, N))
    rows = mc.rows(shape, A).to(DEV)
    word = torch.tensor([5], dtype=torch.int32, device=DEV)
    a12 = fused.sample(rows, SEED, 12, want_probs=True)
    a7 = fused.sample(rows, SEED, 7, step_dev=word, want_probs=True)
    _same(a7, a12)
    assert not torch.equal(fused.sample(rows, SEED, 7)[0], a12[0]), "step 7 and step 12 drew the same 99 actions"
    want = ar.expected_action(ar.draw_u(np.arange(A, dtype=np.uint64), SEED, 7, 5), a7[2][:, 0].cpu().numpy(), False, None)
    assert np.array_equal(a7[0].cpu().numpy(), want)


def test_weights_are_read_in_place_on_every_call():
    shape, N, E = mc.SHAPES[0], 3, 33
    actors = make_actors(shape, N)
    fused = _fused(actors)
    rows = mc.rows(shape, N * E).to(DEV)
    before = fused.sample(rows, SEED, STEP, want_probs=True)
    with torch.no_grad():
        actors[1].fc[1].weight.mul_(0.5)
    after = fused.sample(rows, SEED, STEP, want_probs=True)
    assert torch.equal(after[2][0::N], before[2][0::N]) and torch.equal(after[2][2::N], before[2][2::N])
    assert not torch.equal(after[2][1::N], before[2][1::N])
    _same([x[1::N] for x in after], [x[1::N] for x in _shared(actors[1], rows)])


def _descs(n, K=51, H1=256, H2=256, O=2, size=None, ptr=0x1000, odd=None):
    """n descriptors of one shape; `odd`: (index, field, value) makes one of them differ."""
    arr = (nat.MdrMlp * n)(*[nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, K, H1, H2, O, *([ptr] * 6)) for _ in range(n)])
    if odd is not None:
        setattr(arr[odd[0]], odd[1], odd[2])
    return arr


def test_refused_calls_write_nothing():
    lib = nat.load()
    A = 12
    obs = torch.zeros((A, 129), device=DEV)
    weights = torch.zeros(129 * 257 + 257 * 257, device=DEV)      # real memory behind every pointer of the descriptors
    p = weights.data_ptr()
    inv, uns = nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED
    # (descriptors, nb_nets, obs, ld, nb_rows, action, status)
    cases = [
        (None, 3, True, 51, A, True, inv), (_descs(3, ptr=p), 3, False, 51, A, True, inv), (_descs(3, ptr=p), 3, True, 51, A, False, inv),
        (_descs(3, ptr=p, size=0), 3, True, 51, A, True, inv), (_descs(3, ptr=p, odd=(2, "struct_size", 4)), 3, True, 51, A, True, inv),
        (_descs(3, ptr=p, odd=(1, "w2", None)), 3, True, 51, A, True, inv),
        (_descs(3, ptr=p), 0, True, 51, A, True, inv), (_descs(3, ptr=p), -1, True, 51, A, True, inv),
        (_descs(3, ptr=p), 3, True, 51, -3, True, inv), (_descs(5, ptr=p), 5, True, 51, A, True, inv),      # 12 rows, 5 nets
        (_descs(3, ptr=p), 3, True, 50, A, True, inv),
        (_descs(33, ptr=p), 33, True, 51, 33, True, uns),
        (_descs(3, ptr=p, odd=(1, "hidden1", 255)), 3, True, 51, A, True, uns), (_descs(3, ptr=p, odd=(2, "num_state", 50)), 3, True, 51, A, True, uns),
        (_descs(3, ptr=p, odd=(2, "hidden2", 128)), 3, True, 51, A, True, uns),
        (_descs(3, ptr=p, K=129), 3, True, 129, A, True, uns), (_descs(3, ptr=p, H1=257), 3, True, 51, A, True, uns),
        (_descs(3, ptr=p, H2=257), 3, True, 51, A, True, uns), (_descs(3, ptr=p, O=3), 3, True, 51, A, True, uns),
    ]
    for i, (descs, n, has_obs, ld, rows, has_action, status) in enumerate(cases):
        action = torch.full((64,), 0xEE, dtype=torch.uint8, device=DEV)
        a_prob = torch.full((64,), float("nan"), device=DEV)
        probs = torch.full((64, 2), float("nan"), device=DEV)
        rc = lib.mdr_mlp_actors_sample(descs, n, obs.data_ptr() if has_obs else None, ld, rows, C.c_uint64(1), C.c_uint64(2), None, 0, 0,
                                       action.data_ptr() if has_action else None, a_prob.data_ptr(), probs.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == status, i
        assert bool((action == 0xEE).all()) and bool(a_prob.isnan().all()) and bool(probs.isnan().all()), i
    assert lib.mdr_mlp_actors_sample(_descs(3, ptr=p), 3, obs.data_ptr(), 51, 0, C.c_uint64(1), C.c_uint64(2), None, 0, 0, 0x1000, None, None,
                                     None) == nat.MDR_OK      # no rows: nothing to launch
    from mdr_amd.mlp_actor import FusedMLPActors
    with pytest.raises(ValueError, match="another shape"):
        FusedMLPActors(make_actors(mc.SHAPES[0], 2) + make_actors(mc.SHAPES[4], 1))
    with pytest.raises(ValueError, match="33 nets"):
        FusedMLPActors(make_actors(mc.SHAPES[7], 1) * 33)
    with pytest.raises(ValueError, match="no multiple"):
        _fused(make_actors(mc.SHAPES[7], 3)).sample(torch.zeros((4, 1), device=DEV), 1, 2)
