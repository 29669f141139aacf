"""TarMAC-PPO actor on the GPU: mdr_tarmac_comm against the fp64 banded attention of tests/tarmac_ref.py under its derived bound (every
element, no exclusions), the Philox dead-sender draws, mdr_logits_sample against the project's action stream, the recorded reference
cases through both attention paths, and collect_tarmac_rollout / deploy_policy against an env stepped by hand."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_ref as ar
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = tr.load_cases()


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _comm(q, k, v, E, N, c, out, K=None, V=None, mode=tr.NEIGHBOURS, prob=0.0, seed=0, step=0, step_dev=None, hop=0, q_off=0):
    """mdr_tarmac_comm on 2-D views (rows = agents; the leading dimension is the view's row stride)."""
    import mdr_amd
    lib = mdr_amd.load_native()
    K = q.shape[1] if K is None else K
    V = v.shape[1] if V is None else V
    return lib.mdr_tarmac_comm(_ptr(q, q_off), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), E, N, K, V, c, mode, C.c_float(prob),
                               C.c_uint64(seed), C.c_uint64(step), _ptr(step_dev) if step_dev is not None else None, hop,
                               _ptr(out), out.stride(0), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _inputs(E, N, K, V):
    return tuple(torch.from_numpy(t.reshape(E * N, -1)).to(DEV) for t in tr.comm_inputs(E, N, K, V))


def _worst(out, ref, bound):
    """max over elements of |out - ref| / bound (0 / 0 counts as 0)."""
    err = np.abs(out.astype(np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max())


@pytest.mark.parametrize("shape", tr.COMM_CASES, ids=str)
def test_comm_kernel_holds_the_bound_on_every_element(shape):
    E, N, c, K, V = shape
    q, k, v = _inputs(E, N, K, V)
    out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)      # recycled memory: 0xFF bytes
    assert _comm(q, k, v, E, N, c, out) == 0
    got = out.cpu().numpy().reshape(E, N, V)
    ref, bound = tr.band_attention(*tr.comm_inputs(E, N, K, V), c)
    assert np.isfinite(got).all()
    worst = _worst(got, ref, bound)
    print("%s: worst |comm - ref| / bound_comm = %.3f" % (shape, worst))
    assert worst <= 1.0
    if tr.clamp(c, N) == 0:
        assert torch.equal(out, v)      # a softmax over the receiver alone: the value, bit for bit


def test_comm_mode_none_writes_exact_zeros():
    E, N, K, V = 5, 20, 8, 16
    q, k, v = _inputs(E, N, K, V)
    out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _comm(q, k, v, E, N, 10, out, mode=tr.NONE) == 0
    assert torch.equal(out.view(torch.int32), torch.zeros_like(out, dtype=torch.int32))


def test_comm_packed_projections_and_output_columns():
    E, N, c, K, V = 6, 50, 10, 8, 16
    q, k, v = _inputs(E, N, K, V)
    plain = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _comm(q, k, v, E, N, c, plain) == 0
    qkv = torch.cat([q, k, v], dim=1).contiguous()                      # [A][K + K + V]
    wide = torch.full((E * N, 64 + V + 4), -7.0, dtype=torch.float32, device=DEV)
    assert _comm(qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:], E, N, c, wide[:, 64:64 + V]) == 0
    assert torch.equal(wide[:, 64:64 + V], plain)
    assert bool((wide[:, :64] == -7.0).all()) and bool((wide[:, 64 + V:] == -7.0).all())


def test_comm_argument_checks_launch_nothing():
    from mdr_amd import _native as nat
    E, N = 2, 100
    wide = torch.randn((E * N, 256), dtype=torch.float32, device=DEV)
    out = torch.full((E * N, 80), -7.0, dtype=torch.float32, device=DEV)
    q, k, v = wide[:, :32], wide[:, 32:64], wide[:, 64:144]
    assert _comm(q, k, v, E, N, 10, out, K=6, V=16) == nat.MDR_ERR_UNSUPPORTED          # K no multiple of 4
    assert _comm(q, k, v, E, N, 10, out, K=36, V=16) == nat.MDR_ERR_UNSUPPORTED
    assert _comm(q, k, v, E, N, 10, out, K=8, V=68) == nat.MDR_ERR_UNSUPPORTED          # V > 64
    assert _comm(q, k, v, E, N, 70, out, K=8, V=16) == nat.MDR_ERR_UNSUPPORTED          # c = min(70, 99) > 64
    assert _comm(q, k, v, E, N, 10, out, K=8, V=16, q_off=4) == nat.MDR_ERR_INVALID     # a pointer off 16 bytes
    assert _comm(q, k, v, E, N, 10, out, K=8, V=16, hop=4) == nat.MDR_ERR_INVALID
    assert _comm(q, k, v, E, N, 10, out, K=8, V=16, prob=1.5) == nat.MDR_ERR_INVALID
    assert _comm(q, k, v, E, N, 10, out, K=8, V=16, mode=2) == nat.MDR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert _comm(q, k, v, E, N, 64, out, K=8, V=16) == 0                                # the widest band itself is served
    assert bool((out[:, :16] != -7.0).all()) and bool((out[:, 16:] == -7.0).all())


@pytest.mark.parametrize("shape", tr.DEFECT_CASES, ids=str)
@pytest.mark.parametrize("hop", [0, 1])
def test_comm_defects_follow_the_philox_mask(shape, hop):
    E, N, c, K, V = shape
    q, k, v = _inputs(E, N, K, V)
    host = tr.comm_inputs(E, N, K, V)
    seed = 0x1234567890ABCDEF
    dev7 = torch.tensor([7], dtype=torch.int32, device=DEV)
    for step, step_dev in ((5, None), ((3 << 32) + 0xFFFFFFFE, dev7)):      # the second wraps the low word: no carry into the high one
        out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
        assert _comm(q, k, v, E, N, c, out, prob=0.3, seed=seed, step=step, step_dev=step_dev, hop=hop) == 0
        dead = tr.dead_mask(E, N, 0.3, seed, step, 7 if step_dev is not None else 0, hop)
        assert 0.15 < dead.mean() < 0.45
        ref, bound = tr.band_attention(*host, c, dead=dead)
        worst = _worst(out.cpu().numpy().reshape(E, N, V), ref, bound)
        print("%s hop %d step %#x: worst / bound = %.3f" % (shape, hop, step, worst))
        assert worst <= 1.0
        clean, _ = tr.band_attention(*host, c)
        assert _worst(out.cpu().numpy().reshape(E, N, V), clean, bound) > 1.0      # and the mask matters
    plain = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    none = torch.empty_like(plain)
    alldead = torch.empty_like(plain)
    assert _comm(q, k, v, E, N, c, plain) == 0
    assert _comm(q, k, v, E, N, c, none, prob=0.0, seed=seed, step=5, hop=hop) == 0
    assert _comm(q, k, v, E, N, c, alldead, prob=1.0, seed=seed, step=5, hop=hop) == 0
    assert torch.equal(none, plain)
    assert torch.equal(alldead, v)      # every sender silenced: the receiver hears itself alone


def test_logits_sample_probabilities_draws_and_greedy():
    import mdr_amd
    lib = mdr_amd.load_native()
    A, seed, step = 10007, 0xC0FFEE1234, (2 << 32) + 11
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = (torch.randn((A, 2), generator=g) * 3.0).float()
    logits[:50, 1] = logits[:50, 0]      # ties
    wide = torch.zeros((A, 6), dtype=torch.float32, device=DEV)
    wide[:, :2] = logits.to(DEV)
    dev = torch.tensor([5], dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    l64 = logits.double().numpy()
    p64 = np.stack([1.0 / (1.0 + np.exp(l64[:, 1] - l64[:, 0])), 1.0 / (1.0 + np.exp(l64[:, 0] - l64[:, 1]))], axis=1)
    agents = np.arange(A)
    for src, step_dev in ((logits.to(DEV).contiguous(), None), (wide, dev)):
        action = torch.empty(A, dtype=torch.uint8, device=DEV)
        a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
        probs = torch.empty((A, 2), dtype=torch.float32, device=DEV)
        rc = lib.mdr_logits_sample(_ptr(src), src.stride(0), A, C.c_uint64(seed), C.c_uint64(step), _ptr(step_dev) if step_dev is not None else None,
                                   0, _ptr(action), _ptr(a_prob), _ptr(probs), stream)
        assert rc == 0
        p, act, ap = probs.cpu().numpy(), action.cpu().numpy(), a_prob.cpu().numpy()
        assert ar.contract_ratio(p, p64, False).max() <= 1.0
        u = ar.draw_u(agents, seed, step, 5 if step_dev is not None else 0)      # mdr_actor_sample's stream, through its restatement
        assert np.array_equal(act, ar.expected_action(u, p[:, 0], False, None))
        assert np.array_equal(ap, p[agents, act])
        assert 0.3 < act.mean() < 0.7
    greedy = torch.empty(A, dtype=torch.uint8, device=DEV)
    assert lib.mdr_logits_sample(_ptr(wide), 6, A, C.c_uint64(seed), C.c_uint64(step), None, 1, _ptr(greedy), None, None, stream) == 0
    want = (logits[:, 1] > logits[:, 0]).to(torch.uint8)      # argmax, the first maximum on ties
    assert torch.equal(greedy.cpu(), want) and not bool(greedy[:50].any())
    assert lib.mdr_logits_sample(None, 2, A, C.c_uint64(0), C.c_uint64(0), None, 0, _ptr(greedy), None, None, stream) == -1
    assert lib.mdr_logits_sample(_ptr(wide), 1, A, C.c_uint64(0), C.c_uint64(0), None, 0, _ptr(greedy), None, None, stream) == -1


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("attention", ["band", "dense"])
def test_recorded_reference_cases_end_to_end(name, attention):
    case = CASES[name]
    actor = tr.make_actor(case, attention=attention).to(DEV)
    obs = torch.from_numpy(case["obs"]).to(DEV)
    with torch.no_grad():
        p = actor(obs)
    assert p.shape == case["probs"].shape and p.dtype == torch.float32
    ratio = ar.contract_ratio(p.cpu().numpy(), case["probs"], False).max()
    print("%s / %s: %.3f of the probability contract" % (name, attention, ratio))
    assert ratio <= 1.0
    action, a_prob, probs = actor.sample(obs, seed=9, step=4, want_probs=True)
    if attention == "band":      # the same GEMMs and kernels again; the dense forward() takes torch's softmax instead
        assert torch.equal(probs.view_as(p), p)
    assert ar.contract_ratio(probs.cpu().numpy().reshape(case["probs"].shape), case["probs"], False).max() <= 1.0
    u = ar.draw_u(np.arange(action.numel()), 9, 4)
    assert np.array_equal(action.cpu().numpy(), ar.expected_action(u, probs[:, 0].cpu().numpy(), False, None))


def test_band_path_draws_its_defects_from_philox():
    case = CASES["f51_n50_c10_hops2"]
    actor = tr.make_actor(case, attention="band", defect_prob=0.3).to(DEV)
    obs = torch.from_numpy(case["obs"]).to(DEV)
    seed, step = 77, 12
    dead = [tr.dead_mask(4, case["N"], 0.3, seed, step, hop=h) for h in range(case["hops"])]
    ref = tr.actor_forward(case["sd"], case["obs"], case["c"], case["hops"], dead=dead)
    with torch.no_grad():
        p = actor(obs, seed=seed, step=step)
        p_dense = actor(obs, dead=torch.from_numpy(np.stack(dead)).to(DEV))
    assert ar.contract_ratio(p.cpu().numpy(), ref, False).max() <= 1.0
    assert ar.contract_ratio(p_dense.cpu().numpy(), ref, False).max() <= 1.0
    assert ar.contract_ratio(p.cpu().numpy(), case["probs"], False).max() > 100.0


def _env(E, N, **kw):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=3, **kw)
    env.reset(episode=0)
    return env


def _actor(F, N):
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    torch.manual_seed(11)
    actor, critic = TarMACActor(F), TarMACCritic(N, F)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return actor.to(DEV), critic.to(DEV)


@pytest.mark.parametrize("E,N", [(6, 20), (3, 50)])
def test_collect_tarmac_rollout_and_deploy(E, N):
    from mdr_amd.rollout import collect_tarmac_rollout, deploy_policy, discounted_returns
    T, gamma, seed = 5, 0.9, 5
    env = _env(E, N)
    F = env.obs_vector_length()
    actor, critic = _actor(F, N)
    step0 = env.steps_taken
    ro = collect_tarmac_rollout(env, actor, T, gamma=gamma, critic=critic, seed=seed)
    A = E * N
    assert ro["state"].shape == (T + 1, A, F) and ro["action"].shape == (T, A) and ro["action"].dtype == torch.int64
    assert ro["a_prob"].shape == (T, A) and ro["reward"].shape == (T, A) and ro["return"].shape == (T, A)
    assert ro["done"].dtype == torch.bool and bool(ro["done"][T - 1].all()) and not bool(ro["done"][:T - 1].any())
    assert env.steps_taken == step0 + T
    ref_actor = copy.deepcopy(actor).double()
    twin = _env(E, N)
    agents = np.arange(A)
    for t in range(T):
        assert torch.equal(ro["state"][t], twin.obs_vector("rows").view(A, F))
        with torch.no_grad():      # the reference's dense formula in fp64 on the stored state
            p64 = torch.softmax(ref_actor.dense_logits(ro["state"][t].view(E, N, F).double()), dim=-1).view(A, 2).cpu().numpy()
        act = ro["action"][t].cpu().numpy()
        assert ar.contract_ratio(ro["a_prob"][t].cpu().numpy(), p64[agents, act], False).max() <= 1.0
        # the draw rule on the band path's own p0
        a2, ap2, probs = actor.sample(ro["state"][t].view(E, N, F), seed, step0 + t, want_probs=True)
        assert torch.equal(a2.to(torch.int64), ro["action"][t]) and torch.equal(ap2, ro["a_prob"][t])
        u = ar.draw_u(agents, seed, step0 + t)
        assert np.array_equal(act, ar.expected_action(u, probs[:, 0].cpu().numpy(), False, None))
        assert np.array_equal(ro["a_prob"][t].cpu().numpy(), probs.cpu().numpy()[agents, act])
        twin.step(ro["action"][t].to(torch.uint8).view(E, N))
        assert torch.equal(ro["reward"][t], twin.t["reward"].reshape(-1))
    assert torch.equal(ro["state"][T], twin.obs_vector("rows").view(A, F))
    for name in ("Ta", "Tm", "sso", "flags"):
        assert torch.equal(env.t[name], twin.t[name]), name
    assert env._obs_planes_on and torch.equal(env.t["obs"], twin.t["obs"])      # planes back on and current
    bootstrap = torch.zeros((T, A), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        bootstrap[T - 1] = critic(ro["state"][T].view(E, N, F)).reshape(-1)
    assert bool(bootstrap[T - 1].abs().max() > 0)
    assert torch.equal(ro["return"], discounted_returns(ro["reward"], ro["done"], gamma, bootstrap))
    assert 0.05 < ro["action"].float().mean().item() < 0.95
    # deployment: the same loop, metrics only
    out = deploy_policy(_env(E, N), actor, T, seed=seed)
    hand = _env(E, N)
    total = torch.zeros((E, N), dtype=torch.float32, device=DEV)
    for t in range(T):
        a, _ = actor.sample(hand.obs_vector("rows"), seed, hand.steps_taken)
        _, r, _, _ = hand.step(a.view(E, N))
        total += r
    assert torch.equal(out["reward_sum"], total)
    torch.testing.assert_close(out["reward_sum"], ro["reward"].view(T, E, N).sum(dim=0))      # the same actions as the collection
    assert out["sq_temp_error_sum"].shape == (E,) and out["sq_signal_error_sum"].shape == (E,)
    with pytest.raises(ValueError):
        deploy_policy(_env(E, N), actor, T, use_graph=True)


def test_house_sharded_envs_are_refused():
    from mdr_amd.rollout import collect_tarmac_rollout, deploy_policy
    E, N = 2, 20
    import mdr_amd
    whole = _env(E, N)
    # refused before the env is touched: no episode (and no process group) needed
    shard = mdr_amd.BatchedDemandResponseEnv(whole.config, nb_envs=E, device=DEV, seed=3, house_shard=(0, N), exchange_always=True)
    assert shard.sharded
    actor, _ = _actor(whole.obs_vector_length(), N)
    with pytest.raises(ValueError):
        collect_tarmac_rollout(shard, actor, 2)
    with pytest.raises(ValueError):
        deploy_policy(shard, actor, 2)
    with pytest.raises(ValueError):
        from mdr_amd.rollout import ActorMLP
        collect_tarmac_rollout(whole, ActorMLP(whole.obs_vector_length()).to(DEV), 2)
