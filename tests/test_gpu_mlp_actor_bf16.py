"""mdr_mlp_actor_sample_bf16x3 (csrc/mdr_mlp_actor_bf16.hip) through FusedMLPActor(precision="bf16x3") against the fp64 forward and the
restated Philox draw of tests/actor_ref.py, with the checks of tests/test_gpu_actor_forms.py at layout BF16X3 - the bf16x3 contract:
probabilities within 2e-3 |p| + 2e-5 of fp64 and 5e-6 on average; log(p0 / p1) within the derived running bound + 8 ulp; every action
the restated draw on the kernel's own p0; a_prob the bits of probs[action]; greedy = the sign of the kernel's own logit difference.
Then that it IS the split arithmetic (tests/mlp_actor_bf16_ref.py) and not fp32 under another name, and what the header promises
beside the numbers, as tests/test_gpu_mlp_actor.py holds the fp32 form to it: the same bits whatever the grid, the position in the
batch and the row stride, the device-side step, saturation, weights read in place, refused calls that write nothing; and the loops
that opt into it."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import actor_ref as ar
from tests import mlp_actor_bf16_ref as br
from tests import mlp_actor_cases as mc
from tests.test_gpu_actor_forms import check_outputs
from tests.test_mlp_actor import REFUSED
from tests.test_mlp_actor_bf16 import _refused_call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, STEP = 9, 3
BOTH_FORMS = [mc.SHAPES[0], mc.SHAPES[1]]      # 51 features: the 16-wave form; 121: the 8-wave form


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _fused(shape, greedy=False, precision="bf16x3"):
    from mdr_amd.mlp_actor import FusedMLPActor
    actor = mc.make_actor(shape).to(DEV)
    return actor, FusedMLPActor(actor, greedy=greedy, precision=precision)


@pytest.mark.parametrize("shape", mc.SHAPES, ids=mc.shape_id)
def test_shape_against_fp64_and_its_exact_draw(shape):
    actor, fused = _fused(shape)
    weights = ar.module_weights(actor)
    for A in mc.BATCHES:
        rows = mc.rows(shape, A).to(DEV)
        action, a_prob, probs = fused.sample(rows, SEED, STEP, want_probs=True)
        g_action, g_prob, g_probs = fused.sample(rows, SEED, STEP, greedy=True, want_probs=True)
        assert torch.equal(g_probs, probs), "the greedy form computes other probabilities"
        assert torch.equal(g_prob, probs.gather(1, g_action.long()[:, None])[:, 0])
        with torch.no_grad():
            ref = actor(rows)
        # the 1 % cap on agents inside the bound is a statement about a share: held where a share of the batch means something
        check_outputs("mlp_actor_bf16 %s A=%d" % (mc.shape_id(shape), A), ar.BF16X3, weights, *_np(rows, action, a_prob, probs, g_action),
                      SEED, STEP, ref=ref.cpu().numpy(), cap=A > 1000)


@pytest.mark.parametrize("shape", mc.SHAPES[:7], ids=mc.shape_id)
def test_it_is_the_split_arithmetic_and_not_fp32(shape):
    """p_emu: the stated arithmetic accumulated in float64.  The kernel differs from it by its accumulation order alone - on the CPU an
    fp32-accumulated emulation sits at 0.03-0.054 of the distance between p_emu and fp64 - while an fp32 forward sits at that
    distance itself (0.997-1.002 of it): 0.25 is more than 4x away from both."""
    actor, fused = _fused(shape)
    A = 1029
    rows = mc.rows(shape, A)
    weights = ar.module_weights(actor)
    _, p0, p1, _ = ar.forward64(*weights, rows.numpy(), layout=ar.BF16X3)
    p64 = np.stack([p0, p1], 1)
    p_emu = br.forward(weights, rows.numpy(), acc=np.float64).astype(np.float64)
    probs = fused.sample(rows.to(DEV), SEED, STEP, want_probs=True)[2]
    exact = _fused(shape, precision="fp32")[1].sample(rows.to(DEV), SEED, STEP, want_probs=True)[2]
    p_kernel = probs.cpu().numpy().astype(np.float64)
    near, far = float(np.abs(p_kernel - p_emu).mean()), float(np.abs(p64 - p_emu).mean())
    fp32_near = float(np.abs(exact.cpu().numpy().astype(np.float64) - p_emu).mean())
    print("MLP_ACTOR_BF16_IS %s |kernel - emu|=%.3e |fp64 - emu|=%.3e ratio=%.4f; the fp32 form: %.4f" % (mc.shape_id(shape), near, far, near / far, fp32_near / far))
    assert near <= 0.25 * far
    assert not torch.equal(probs, exact)


@pytest.mark.parametrize("shape", BOTH_FORMS, ids=mc.shape_id)
def test_the_grid_does_not_change_a_bit(shape):
    _, fused = _fused(shape)
    rows = mc.rows(shape, 5000).to(DEV)
    outs = [fused.sample(rows, SEED, STEP, want_probs=True, max_workgroups=mw) for mw in (1, 3, 0)]
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)
    assert bool(torch.isfinite(outs[0][2]).all())


@pytest.mark.parametrize("shape", BOTH_FORMS, ids=mc.shape_id)
def test_the_position_in_the_batch_does_not_change_a_bit(shape):
    _, fused = _fused(shape)
    rows = mc.rows(shape, 1029).to(DEV)
    _, _, whole = fused.sample(rows, SEED, STEP, want_probs=True)
    _, _, alone = fused.sample(rows[500:517].contiguous(), SEED, STEP, want_probs=True)
    assert torch.equal(alone, whole[500:517])
    _, _, view = fused.sample(rows[500:517], SEED, STEP, want_probs=True)      # 4-byte aligned rows inside the batch
    assert torch.equal(view, whole[500:517])


@pytest.mark.parametrize("shape", BOTH_FORMS + [mc.SHAPES[4]], ids=mc.shape_id)
def test_a_row_stride_beyond_f_reads_no_pad_column(shape):
    _, fused = _fused(shape)
    F, A = shape[0], 1029
    rows = mc.rows(shape, A).to(DEV)
    wide = torch.full((A, F + 5), float("nan"), device=DEV)
    wide[:, :F] = rows
    want = fused.sample(rows, SEED, STEP, want_probs=True)
    got = fused.sample(wide[:, :F], SEED, STEP, want_probs=True)
    for x, y in zip(want, got):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(got[2]).all())


def _raw(fused, rows, seed, step, step_dev, greedy, action, a_prob, probs):
    from mdr_amd import _learner as L
    desc = L.mlp_desc(L.fc_layers(fused.module))
    rc = nat.load().mdr_mlp_actor_sample_bf16x3(C.byref(desc), L.ptr(rows), rows.stride(0), rows.shape[0], C.c_uint64(seed), C.c_uint64(step),
                                                L.ptr(step_dev), greedy, 0, L.ptr(action), L.ptr(a_prob), L.ptr(probs), L.stream(rows.device))
    assert rc == nat.MDR_OK
    return action


def test_the_device_side_step_and_null_outputs():
    shape = mc.SHAPES[0]
    _, fused = _fused(shape)
    rows = mc.rows(shape, 1029).to(DEV)
    word = torch.tensor([5], dtype=torch.int32, device=DEV)
    a12, p12, probs12 = fused.sample(rows, SEED, 12, want_probs=True)
    a7, p7, probs7 = fused.sample(rows, SEED, 7, step_dev=word, want_probs=True)
    assert torch.equal(a7, a12) and torch.equal(p7, p12) and torch.equal(probs7, probs12)
    a_other, _ = fused.sample(rows, SEED, 7)
    assert not torch.equal(a_other, a12), "step 7 and step 12 drew the same 1029 actions"
    want = ar.expected_action(ar.draw_u(np.arange(1029, dtype=np.uint64), SEED, 7, 5), probs7[:, 0].cpu().numpy(), False, None)
    assert np.array_equal(a7.cpu().numpy(), want)
    bare = _raw(fused, rows, SEED, 7, word, 0, torch.full((1029,), 9, dtype=torch.uint8, device=DEV), None, None)
    assert torch.equal(bare, a12)
    bare = _raw(fused, rows, SEED, 12, None, 0, torch.full((1029,), 9, dtype=torch.uint8, device=DEV), None, None)
    assert torch.equal(bare, a12)


@pytest.mark.parametrize("F", [51, 121])
def test_an_action_of_probability_zero_is_never_drawn(F):
    from mdr_amd.maddpg import DDPGNetworkMLP
    from mdr_amd.mlp_actor import FusedMLPActor
    actor = DDPGNetworkMLP(F, 2, 256).to(DEV)
    with torch.no_grad():
        for lin in actor.fc:
            lin.weight.zero_()
            lin.bias.zero_()
        actor.fc[2].bias.copy_(torch.tensor([200.0, 0.0]))
    A = 65536
    rows = torch.randn((A, F), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    action, a_prob, probs = FusedMLPActor(actor, precision="bf16x3").sample(rows, 11, 41, want_probs=True)
    assert bool((probs[:, 0] == 1.0).all()) and bool((probs[:, 1] == 0.0).all())
    assert int(action.sum()) == 0 and bool((a_prob == 1.0).all())


def test_weights_are_read_in_place_on_every_call():
    shape = mc.SHAPES[0]
    actor, fused = _fused(shape)
    rows = mc.rows(shape, 1029).to(DEV)
    before = fused.sample(rows, SEED, STEP, want_probs=True)
    with torch.no_grad():
        actor.fc[1].weight.mul_(0.5)
    action, a_prob, probs = fused.sample(rows, SEED, STEP, want_probs=True)
    assert not torch.equal(probs, before[2])
    g_action, _ = fused.sample(rows, SEED, STEP, greedy=True)
    check_outputs("mlp_actor_bf16 in-place %s" % mc.shape_id(shape), ar.BF16X3, ar.module_weights(actor), *_np(rows, action, a_prob, probs, g_action),
                  SEED, STEP, cap=False)      # the halved layer moves the logits towards 0: the cap belongs to the network built for it


def test_refused_calls_write_nothing():
    lib = nat.load()
    A = 16
    obs = torch.zeros((A, 129), device=DEV)
    for kw, status in REFUSED:
        kw = dict(kw)
        action = torch.full((A,), 7, dtype=torch.uint8, device=DEV)
        a_prob = torch.full((A,), -3.0, device=DEV)
        probs = torch.full((A, 2), -5.0, device=DEV)
        weights = torch.zeros(129 * 257 + 257 * 257, device=DEV)      # real memory behind every pointer of the descriptor
        o = None if "obs" in kw and kw.pop("obs") is None else obs.data_ptr()
        a = None if "action" in kw and kw.pop("action") is None else action.data_ptr()
        rc = _refused_call(lib, o, a, a_prob.data_ptr(), probs.data_ptr(), A=A, ptr=weights.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream, **kw)
        torch.cuda.synchronize()
        assert rc == status, kw
        assert bool((action == 7).all()) and bool((a_prob == -3.0).all()) and bool((probs == -5.0).all()), kw


# ---- the loops that opt into it: 8 envs x 20 houses, the reference's 51 features and its 256-256 actor
E, N = 8, 20


def _env():
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=11)
    env.reset(episode=0)
    return env


def _ddpg_actor(seed=4):
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(seed)
    actor = DDPGNetworkMLP(51, 2, 256).to(DEV)
    with torch.no_grad():      # spread the probabilities: the default init leaves them all near one value
        actor.fc[2].weight.mul_(8.0)
    return actor


def test_collect_maddpg_transitions_acts_through_the_bf16x3_kernel():
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import collect_maddpg_transitions
    actor = _ddpg_actor()
    env = _env()
    seed, T = 5, 3
    got = collect_maddpg_transitions(env, actor, T, random_steps_left=1, seed=seed, actor_backend="hip-bf16x3")
    assert got["state"].shape == (T + 1, E, N, 51) and got["action"].shape == (T, E, N) and env.steps_taken == T
    fused, exact = FusedMLPActor(actor, precision="bf16x3"), FusedMLPActor(actor)
    agents = np.arange(E * N, dtype=np.uint64)
    for t in (1, 2):      # env.steps_taken was t when step t acted
        rows = got["state"][t].view(E * N, 51)
        action, a_prob, probs = fused.sample(rows, seed, t, want_probs=True)
        assert torch.equal(action.to(torch.int64), got["action"][t].view(-1)), "step %d is not the bf16x3 kernel on the stored rows" % t
        want = ar.expected_action(ar.draw_u(agents, seed, t), probs[:, 0].cpu().numpy(), False, None)
        assert np.array_equal(got["action"][t].view(-1).cpu().numpy(), want)
        assert torch.equal(a_prob, probs.gather(1, action.long()[:, None])[:, 0])
        assert not torch.equal(probs, exact.sample(rows, seed, t, want_probs=True)[2])
    assert 0 < int(got["action"][1:].sum()) < 2 * E * N      # both actions occur
    with pytest.raises(ValueError, match="fp32 only"):
        collect_maddpg_transitions(env, [actor] * N, 1, actor_backend="hip-bf16x3")


def test_deploy_policy_takes_the_greedy_bf16x3_kernel():
    from mdr_amd.maddpg import GreedyDDPGActor
    from mdr_amd.mlp_actor import FusedMLPActor
    from mdr_amd.rollout import deploy_policy
    actor = _ddpg_actor()
    T = 4
    policy = GreedyDDPGActor(actor, backend="hip-bf16x3")
    assert policy._fused.precision == "bf16x3" and policy._fused.greedy
    out = deploy_policy(_env(), policy, T)
    env = _env()
    fused = FusedMLPActor(actor, precision="bf16x3", greedy=True)
    want = {"reward_sum": torch.zeros((E, N), dtype=torch.float32, device=DEV), "sq_temp_error_sum": torch.zeros(E, dtype=torch.float64, device=DEV),
            "sq_signal_error_sum": torch.zeros(E, dtype=torch.float64, device=DEV)}
    obs = torch.empty((E, N, 51), dtype=torch.float32, device=DEV)
    picks = 0
    for t in range(T):
        env.obs_vector("rows", out=obs)
        act, _ = fused.sample(obs.view(E * N, 51), 0, t)
        picks += int(act.sum())
        _, r, _, info = env.step(act.view(E, N))
        want["reward_sum"] += r
        d = (env.t["Ta"] - env.t["target"]).double()
        want["sq_temp_error_sum"] += (d * d).sum(dim=1)
        want["sq_signal_error_sum"] += (env.reg_signal() - info["cluster_hvac_power"]) ** 2
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert 0 < picks < T * E * N      # both actions occur
