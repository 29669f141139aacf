"""FusedTarMACActor / mdr_tarmac_actor_sample (csrc/mdr_tarmac_mlp.hip) against the fp64 actor of tests/tarmac_ref.py, the recorded
reference cases and the draw of tests/actor_ref.py.  The one tolerance is the project's probability contract:
actor_ref.contract_ratio(p, ref64, False) <= 1.  Every case prints the share of the contract it used."""
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


def _fused(actor):
    from mdr_amd.tarmac import FusedTarMACActor
    return FusedTarMACActor.from_module(actor)


def _actor(F, H=64, K=8, V=16, c=10, hops=1, seed=11, **kw):
    """torch's default init with the weights doubled, as tests/test_gpu_tarmac.py builds its actors: p0 spreads over (0, 1)."""
    from mdr_amd.tarmac import TarMACActor
    torch.manual_seed(seed)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=c, num_hops=hops, **kw)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return actor.to(DEV)


def _sd(actor):
    return {k: v.detach().cpu().numpy() for k, v in actor.state_dict().items()}


def _obs(E, N, F, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn((E, N, F), generator=g)


def _check_sample(fused, obs_dev, ref64, seed, step, what):
    """The contract on all probabilities, the draw on the kernel's own p0, a_prob = probs[agent, action]."""
    action, a_prob, probs = fused.sample(obs_dev, seed, step, want_probs=True)
    A = obs_dev.shape[0] * obs_dev.shape[1]
    p = probs.cpu().numpy()
    assert p.shape == (A, 2) and action.shape == (A,) and action.dtype == torch.uint8
    if ref64 is not None:
        ratio = ar.contract_ratio(p, np.asarray(ref64).reshape(A, 2), False).max()
        print("%s: %.4f of the probability contract" % (what, ratio))
        assert ratio <= 1.0
    agents = np.arange(A)
    act = action.cpu().numpy()
    assert np.array_equal(act, ar.expected_action(ar.draw_u(agents, seed, step), p[:, 0], False, None))
    assert np.array_equal(a_prob.cpu().numpy(), p[agents, act])
    return p, act


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_reference_cases(name):
    case = CASES[name]
    fused = _fused(tr.make_actor(case).to(DEV))
    obs = torch.from_numpy(case["obs"]).to(DEV)
    _check_sample(fused, obs, case["probs"], 9, 4, name)
    p = fused.probs(obs)
    assert p.shape == case["probs"].shape and ar.contract_ratio(p.cpu().numpy(), case["probs"], False).max() <= 1.0


# (E, N): a single agent; A = 15, less than one tile; exactly one tile; A = 77, a partial last tile and tiles that span envs; several
# attention tiles per env
SHAPES = [(1, 1), (3, 5), (1, 16), (7, 11), (2, 300)]


@pytest.mark.parametrize("hops", [1, 2, 4])
@pytest.mark.parametrize("E,N", SHAPES)
def test_reference_sizes_against_fp64(E, N, hops):
    actor = _actor(51, hops=hops)
    obs = _obs(E, N, 51, seed=hops)
    ref = tr.actor_forward(_sd(actor), obs.numpy(), 10, hops)
    _check_sample(_fused(actor), obs.to(DEV), ref, 5, 17, "E%d N%d hops%d" % (E, N, hops))


@pytest.mark.parametrize("F,H,K,V", [(64, 48, 16, 32), (3, 64, 4, 4)])
@pytest.mark.parametrize("hops", [1, 2])
def test_other_block_counts_against_fp64(F, H, K, V, hops):
    E, N = 7, 11
    actor = _actor(F, H, K, V, hops=hops)
    obs = _obs(E, N, F)
    ref = tr.actor_forward(_sd(actor), obs.numpy(), 10, hops)
    _check_sample(_fused(actor), obs.to(DEV), ref, 5, 17, "F%d H%d K%d V%d hops%d" % (F, H, K, V, hops))


def test_without_communication_and_mode_none():
    E, N = 7, 11
    for kw, ref_kw in ((dict(with_comm=False), dict(with_comm=False)), (dict(comm_mode="none"), dict(mode=tr.NONE))):
        actor = _actor(51, **kw)
        obs = _obs(E, N, 51)
        ref = tr.actor_forward(_sd(actor), obs.numpy(), 10, 1, **ref_kw)
        _check_sample(_fused(actor), obs.to(DEV), ref, 5, 17, str(kw))


def test_grid_stride_every_wavefront_takes_two_tiles_and_a_partial_pass():
    """The launcher's grid rule (csrc/mdr_tarmac_mlp.hip, as mdr_actor_sample): min(ceil(tiles / 16), CUs) workgroups of 16 waves,
    16 agents per wave - one pass of the grid covers CUs * 256 agents, 65,536 on 256 CUs.  E is chosen so that A = 50 E is two full
    passes plus a partial third: every wavefront takes at least two tiles, some three.  Envs are independent: the fp64 reference
    runs on the first env, the last, and the envs on either side of each pass boundary; the draw is checked for every agent."""
    N = 50
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_pass = cus * 16 * 16
    E = (2 * per_pass + per_pass // 16) // N + 1
    A = E * N
    assert 2 * per_pass < A < 3 * per_pass
    actor = _actor(51, hops=2)
    g = torch.Generator(device=DEV).manual_seed(3)
    obs = torch.randn((E, N, 51), generator=g, device=DEV)
    p, _ = _check_sample(_fused(actor), obs, None, 21, 3, "grid stride")
    envs = sorted({0, E - 1, *(b // N + d for b in (per_pass, 2 * per_pass) for d in (-1, 0, 1))})
    ref = tr.actor_forward(_sd(actor), obs[envs].cpu().numpy(), 10, 2)
    got = p.reshape(E, N, 2)[envs]
    ratio = ar.contract_ratio(got, ref, False).max()
    print("grid stride, envs %s: %.4f of the probability contract" % (envs, ratio))
    assert ratio <= 1.0


def test_defects_are_drawn_from_philox():
    E, N, hops, seed, step = 5, 50, 2, 77, 12
    actor = _actor(51, hops=hops, comm_defect_prob=0.3)
    obs = _obs(E, N, 51)
    dead = [tr.dead_mask(E, N, 0.3, seed, step, hop=h) for h in range(hops)]
    ref = tr.actor_forward(_sd(actor), obs.numpy(), 10, hops, dead=dead)
    _check_sample(_fused(actor), obs.to(DEV), ref, seed, step, "defects")
    healthy = copy.deepcopy(actor)
    healthy.comm_defect_prob = 0.0
    p = _fused(healthy).probs(obs.to(DEV), seed, step).cpu().numpy()
    assert ar.contract_ratio(p, ref, False).max() > 100.0


def test_step_dev_and_greedy():
    E, N, seed, step = 7, 11, 5, 40
    A = E * N
    actor = _actor(51)
    fused = _fused(actor)
    obs = _obs(E, N, 51).to(DEV)
    step_dev = torch.tensor([9], dtype=torch.int32, device=DEV)
    a_dev, ap_dev, p_dev = fused.sample(obs, seed, step, step_dev=step_dev, want_probs=True)
    a_sum, ap_sum, p_sum = fused.sample(obs, seed, step + 9, want_probs=True)
    assert torch.equal(a_dev, a_sum) and torch.equal(ap_dev, ap_sum) and torch.equal(p_dev, p_sum)
    u = ar.draw_u(np.arange(A), seed, step, step_dev=9)
    assert np.array_equal(a_dev.cpu().numpy(), ar.expected_action(u, p_dev[:, 0].cpu().numpy(), False, None))
    a_plain, _ = fused.sample(obs, seed, step)
    assert not torch.equal(a_plain, a_dev)      # 77 draws: another step, other actions
    a_g, ap_g, p_g = fused.sample(obs, seed, step, greedy=True, want_probs=True)
    assert torch.equal(p_g, p_dev)
    d, normal = ar.kernel_logit_difference(p_g.cpu().numpy())
    assert normal.all()
    # p0 >= p1 iff d >= 0 on the kernel's own probabilities (p0 == p1 only at d == 0: the first maximum)
    pg = p_g.cpu().numpy()
    want = np.where(pg[:, 0] >= pg[:, 1], 0, 1).astype(np.uint8)
    assert np.array_equal(want, ar.expected_action(None, None, True, d))
    assert np.array_equal(a_g.cpu().numpy(), want)
    assert np.array_equal(ap_g.cpu().numpy(), pg[np.arange(A), want])
    a_g2, _ = fused.sample(obs, seed + 1, step + 5, greedy=True)      # no draw: the seed does not matter
    assert torch.equal(a_g, a_g2)
    with pytest.raises(ValueError):
        fused.sample(obs, seed, step, step_dev=step_dev.long())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def test_c_abi_directly():
    """mdr_tarmac_actor_sample through ctypes with caller-owned workspace: bit for bit FusedTarMACActor.sample; refusals launch
    nothing and touch no output."""
    from mdr_amd import _native as nat
    from mdr_amd.tarmac import MdrTarmacActor
    lib = nat.load()
    E, N, seed, step = 7, 11, 5, 40
    A = E * N
    actor = _actor(51, hops=2)
    fused = _fused(actor)
    obs = _obs(E, N, 51).to(DEV)
    want = fused.sample(obs, seed, step, want_probs=True)
    st = MdrTarmacActor.from_buffer_copy(fused._pack())
    nbytes = lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), A)
    assert nbytes == A * 4 * (64 + 16 + 8 + 8 + 16 + 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def outputs():
        return (torch.full((A,), 7, dtype=torch.uint8, device=DEV), torch.full((A,), -3.0, device=DEV), torch.full((A, 2), -3.0, device=DEV))

    def call(s, obs_t=obs, ws_t=ws, out=None):
        action, a_prob, probs = out
        return lib.mdr_tarmac_actor_sample(C.byref(s) if s is not None else None, _ptr(obs_t), E, N, C.c_uint64(seed), C.c_uint64(step), None,
                                           _ptr(ws_t), _ptr(action), _ptr(a_prob), _ptr(probs), stream)

    out = outputs()
    assert call(st, out=out) == 0
    for got, ref in zip(out, want):
        assert torch.equal(got, ref)

    def untouched(rc_want, s, **kw):
        o = outputs()
        assert call(s, out=o, **kw) == rc_want
        torch.cuda.synchronize()
        assert bool((o[0] == 7).all()) and bool((o[1] == -3.0).all()) and bool((o[2] == -3.0).all())

    untouched(-1, None)
    untouched(-1, st, obs_t=None)
    untouched(-1, st, ws_t=None)
    o = outputs()
    assert call(st, out=(None, o[1], o[2])) == -1 and bool((o[1] == -3.0).all()) and bool((o[2] == -3.0).all())
    bad = MdrTarmacActor.from_buffer_copy(st)
    bad.frag_encode = None
    untouched(-1, bad)
    small = MdrTarmacActor.from_buffer_copy(st)
    small.struct_size = C.sizeof(MdrTarmacActor) - 8
    untouched(-1, small)
    k32 = MdrTarmacActor.from_buffer_copy(st)
    k32.num_key = 32
    untouched(-4, k32)
    f65 = MdrTarmacActor.from_buffer_copy(st)
    f65.num_state = 65
    untouched(-4, f65)


def _env(E, N, **kw):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=3, **kw)
    env.reset(episode=0)
    return env


@pytest.mark.parametrize("E,N", [(6, 20), (3, 50)])
def test_collect_tarmac_rollout_with_the_fused_actor(E, N):
    from mdr_amd.rollout import collect_tarmac_rollout
    T, seed = 5, 5
    env = _env(E, N)
    F = env.obs_vector_length()
    actor = _actor(F)
    fused = _fused(actor)
    step0 = env.steps_taken
    ro = collect_tarmac_rollout(env, fused, T, gamma=0.9, seed=seed)
    A = E * N
    assert ro["state"].shape == (T + 1, A, F) and ro["action"].shape == (T, A) and env.steps_taken == step0 + T
    ref_actor = copy.deepcopy(actor).double()
    twin = _env(E, N)
    agents = np.arange(A)
    worst = 0.0
    for t in range(T):
        assert torch.equal(ro["state"][t], twin.obs_vector("rows").view(A, F))
        with torch.no_grad():      # the reference's dense formula in fp64 on the stored state
            p64 = torch.softmax(ref_actor.dense_logits(ro["state"][t].view(E, N, F).double()), dim=-1).view(A, 2).cpu().numpy()
        act = ro["action"][t].cpu().numpy()
        worst = max(worst, ar.contract_ratio(ro["a_prob"][t].cpu().numpy(), p64[agents, act], False).max())
        a2, ap2, probs = fused.sample(ro["state"][t].view(E, N, F), seed, step0 + t, want_probs=True)
        assert torch.equal(a2.to(torch.int64), ro["action"][t]) and torch.equal(ap2, ro["a_prob"][t])
        assert np.array_equal(act, ar.expected_action(ar.draw_u(agents, seed, step0 + t), probs[:, 0].cpu().numpy(), False, None))
        twin.step(ro["action"][t].to(torch.uint8).view(E, N))
        assert torch.equal(ro["reward"][t], twin.t["reward"].reshape(-1))
    print("rollout E%d N%d: %.4f of the probability contract" % (E, N, worst))
    assert worst <= 1.0
    assert torch.equal(ro["state"][T], twin.obs_vector("rows").view(A, F))
    for name in ("Ta", "Tm", "sso", "flags"):
        assert torch.equal(env.t[name], twin.t[name]), name
    assert env._obs_planes_on and torch.equal(env.t["obs"], twin.t["obs"])      # planes back on and current
    assert 0.05 < ro["action"].float().mean().item() < 0.95


def test_captured_deployment_equals_the_eager_one():
    """table_steps = 16 and 40 steps: the replays cross two table refills."""
    import mdr_amd
    from mdr_amd.rollout import deploy_policy
    E, N, T = 4, 20, 40
    cfg = _env(1, N).config
    envs = [mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=2, table_steps=16, graph_mode=True) for _ in range(3)]
    for e in envs:
        e.reset(episode=0)
    actor = _actor(envs[0].obs_vector_length())
    fused = _fused(actor)
    eager = deploy_policy(envs[0], fused, T, seed=7, use_graph=False)
    graph = deploy_policy(envs[1], fused, T, seed=7, use_graph=True)
    for name in ("reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"):
        assert torch.equal(eager[name], graph[name]), name
    assert bool(eager["reward_sum"].abs().sum() > 0)
    with pytest.raises(ValueError):
        deploy_policy(envs[2], actor, T, use_graph=True)


def test_house_sharded_envs_are_refused_for_both_actors():
    import mdr_amd
    from mdr_amd.rollout import collect_tarmac_rollout, deploy_policy
    E, N = 2, 20
    whole = _env(E, N)
    shard = mdr_amd.BatchedDemandResponseEnv(whole.config, nb_envs=E, device=DEV, seed=3, house_shard=(0, N), exchange_always=True)
    assert shard.sharded
    actor = _actor(whole.obs_vector_length())
    for policy in (actor, _fused(actor)):
        with pytest.raises(ValueError):
            collect_tarmac_rollout(shard, policy, 2)
        with pytest.raises(ValueError):
            deploy_policy(shard, policy, 2)
