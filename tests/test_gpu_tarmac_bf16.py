"""FusedTarMACActor(precision="bf16x3") / mdr_tarmac_actor_sample with MDR_TARMAC_BF16X3 (csrc/mdr_tarmac_mlp_bf16.hip) against the
fp64 actor of tests/tarmac_ref.py, the recorded reference cases and the draw of tests/actor_ref.py.  The one tolerance is the
project's bf16x3 probability contract: actor_ref.contract_ratio(p, ref64, True) <= 1 - which tests/test_tarmac_bf16.py shows a forward
without either cross term misses on every input used here.  Every case prints the share of the contract it used; the CPU emulation of
tests/tarmac_bf16_ref.py uses 0.005-0.023 of it on the same inputs."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_ref as ar
from tests import tarmac_bf16_ref as br
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = tr.load_cases()
SYNTHETIC = br.synthetic_inputs()


def _fused(actor, precision="bf16x3"):
    from mdr_amd.tarmac import FusedTarMACActor
    fused = FusedTarMACActor.from_module(actor, precision=precision)
    assert fused.precision == precision
    return fused


def _actor(F, **kw):
    return br.make_actor(F, **kw).to(DEV)


def _check_sample(fused, obs_dev, ref64, seed, step, what):
    """The contract on all probabilities, the draw on the kernel's own p0, a_prob = probs[agent, action]."""
    action, a_prob, probs = fused.sample(obs_dev, seed, step, want_probs=True)
    A = obs_dev.shape[0] * obs_dev.shape[1]
    p = probs.cpu().numpy()
    assert p.shape == (A, 2) and action.shape == (A,) and action.dtype == torch.uint8
    if ref64 is not None:
        ratio = ar.contract_ratio(p, np.asarray(ref64).reshape(A, 2), True).max()
        print("%s: %.4f of the bf16x3 probability contract" % (what, ratio))
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
    assert p.shape == case["probs"].shape and ar.contract_ratio(p.cpu().numpy(), case["probs"], True).max() <= 1.0


def test_all_seven_recorded_cases_are_there():
    assert len(CASES) == 7


# the tile corners for 32 agents per wavefront, the other block counts (the general form, the odd half k-step), with_comm=False and
# comm_mode="none": tests/tarmac_bf16_ref.py builds them, tests/test_tarmac_bf16.py judges them on the CPU
@pytest.mark.parametrize("name", sorted(n for n in SYNTHETIC if n != "defects"))
def test_synthetic_inputs_against_fp64(name):
    actor, obs, ref, _ = br.build_input(SYNTHETIC[name])
    _check_sample(_fused(actor.to(DEV)), obs.to(DEV), ref, 5, 17, name)


def test_the_inputs_cover_what_they_must():
    shapes = {(s["E"], s["N"], s["kw"].get("hops", 1)) for s in SYNTHETIC.values() if s["kw"]["F"] == 51 and len(s["kw"]) <= 2}
    assert {(1, 1, 1), (3, 5, 1), (1, 16, 1), (1, 32, 1), (1, 33, 1), (7, 11, 1), (2, 300, 1), (7, 11, 2), (7, 11, 4), (2, 300, 2), (2, 300, 4)} <= shapes
    blocks = {(s["kw"]["F"], s["kw"].get("H"), s["kw"].get("K"), s["kw"].get("V"), s["kw"].get("hops")) for s in SYNTHETIC.values()}
    assert {(64, 48, 16, 32, 1), (64, 48, 16, 32, 2), (3, 64, 4, 4, 1), (3, 64, 4, 4, 2)} <= blocks


def test_grid_stride_every_wavefront_takes_two_tiles_and_a_partial_pass():
    """tarmac_bf16_ref.grid_stride_input: A = 50 E is two full passes of the grid plus a partial third.  Envs are independent: the fp64
    reference runs on the first env, the last, and the envs on either side of each pass boundary; the draw is checked for every agent."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    E, per_pass, envs = br.grid_stride_input(cus)
    N = br.GRID_N
    assert per_pass == cus * 8 * 32 and 2 * per_pass < E * N < 3 * per_pass
    actor = _actor(51, hops=br.GRID_HOPS)
    obs = br.grid_stride_obs(E, DEV)
    p, _ = _check_sample(_fused(actor), obs, None, 21, 3, "grid stride")
    ref = tr.actor_forward(br.state_dict(actor), obs[envs].cpu().numpy(), 10, br.GRID_HOPS)
    got = p.reshape(E, N, 2)[envs]
    ratio = ar.contract_ratio(got, ref, True).max()
    print("grid stride, envs %s: %.4f of the bf16x3 probability contract" % (envs, ratio))
    assert ratio <= 1.0


def test_defects_are_drawn_from_philox():
    d = br.DEFECTS
    actor, obs, ref, _ = br.build_input(SYNTHETIC["defects"])
    actor = actor.to(DEV)
    _check_sample(_fused(actor), obs.to(DEV), ref, d["seed"], d["step"], "defects")
    healthy = copy.deepcopy(actor)
    healthy.comm_defect_prob = 0.0
    p = _fused(healthy).probs(obs.to(DEV), d["seed"], d["step"]).cpu().numpy()
    assert ar.contract_ratio(p, ref, True).max() > 1.0


def test_step_dev_and_greedy():
    E, N, seed, step = 7, 11, 5, 40
    A = E * N
    actor = _actor(51)
    fused = _fused(actor)
    obs = br.make_obs(E, N, 51).to(DEV)
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
    """mdr_tarmac_actor_sample with precision = 1 through ctypes and a caller-owned workspace: bit for bit FusedTarMACActor.sample;
    precision = 2 is refused with nothing launched and no output touched; the default precision is fp32, bit for bit."""
    from mdr_amd import _native as nat
    from mdr_amd.tarmac import FusedTarMACActor, MdrTarmacActor
    lib = nat.load()
    E, N, seed, step = 7, 11, 5, 40
    A = E * N
    actor = _actor(51, hops=2)
    fused = _fused(actor)
    obs = br.make_obs(E, N, 51).to(DEV)
    want = fused.sample(obs, seed, step, want_probs=True)
    st = MdrTarmacActor.from_buffer_copy(fused._pack())
    assert st.precision == 1
    for part, name in enumerate(("frag_encode", "frag_proj", "frag_msg", "frag_head")):
        assert lib.mdr_tarmac_frag_words(C.byref(st), part) == fused._tensors[name].numel()
    nbytes = lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), A)
    assert nbytes == A * 4 * (64 + 16 + 8 + 8 + 16 + 64)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def outputs():
        return (torch.full((A,), 7, dtype=torch.uint8, device=DEV), torch.full((A,), -3.0, device=DEV), torch.full((A, 2), -3.0, device=DEV))

    def call(s, out):
        action, a_prob, probs = out
        return lib.mdr_tarmac_actor_sample(C.byref(s), _ptr(obs), E, N, C.c_uint64(seed), C.c_uint64(step), None, _ptr(ws), _ptr(action),
                                           _ptr(a_prob), _ptr(probs), stream)

    out = outputs()
    assert call(st, out) == 0
    for got, ref in zip(out, want):
        assert torch.equal(got, ref)
    for precision in (2, -1):
        bad = MdrTarmacActor.from_buffer_copy(st)
        bad.precision = precision
        o = outputs()
        assert call(bad, o) == -1      # MDR_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((o[0] == 7).all()) and bool((o[1] == -3.0).all()) and bool((o[2] == -3.0).all())
    plain = FusedTarMACActor.from_module(actor).sample(obs, seed, step, want_probs=True)
    fp32 = FusedTarMACActor.from_module(actor, precision="fp32").sample(obs, seed, step, want_probs=True)
    for a, b in zip(plain, fp32):
        assert torch.equal(a, b)
    assert not torch.equal(plain[2], want[2])      # and bf16x3 is another arithmetic


def test_repack_on_parameter_change():
    actor = _actor(51)
    fused = _fused(actor)
    obs = br.make_obs(7, 11, 51).to(DEV)
    before = fused.probs(obs).clone()
    with torch.no_grad():
        actor.obs2hidden[0].weight.mul_(0.5)
    after = fused.probs(obs)
    assert not torch.equal(before, after)
    ref = tr.actor_forward(br.state_dict(actor), obs.cpu().numpy(), 10, 1)
    assert ar.contract_ratio(after.cpu().numpy(), ref, True).max() <= 1.0


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
def test_collect_tarmac_rollout_with_the_bf16x3_actor(E, N):
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
        worst = max(worst, ar.contract_ratio(ro["a_prob"][t].cpu().numpy(), p64[agents, act], True).max())
        a2, ap2, probs = fused.sample(ro["state"][t].view(E, N, F), seed, step0 + t, want_probs=True)
        assert torch.equal(a2.to(torch.int64), ro["action"][t]) and torch.equal(ap2, ro["a_prob"][t])
        assert np.array_equal(act, ar.expected_action(ar.draw_u(agents, seed, step0 + t), probs[:, 0].cpu().numpy(), False, None))
        twin.step(ro["action"][t].to(torch.uint8).view(E, N))
        assert torch.equal(ro["reward"][t], twin.t["reward"].reshape(-1))
    print("rollout E%d N%d: %.4f of the bf16x3 probability contract" % (E, N, worst))
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
    envs = [mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=2, table_steps=16, graph_mode=True) for _ in range(2)]
    for e in envs:
        e.reset(episode=0)
    actor = _actor(envs[0].obs_vector_length())
    fused = _fused(actor)
    eager = deploy_policy(envs[0], fused, T, seed=7, use_graph=False)
    graph = deploy_policy(envs[1], fused, T, seed=7, use_graph=True)
    for name in ("reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"):
        assert torch.equal(eager[name], graph[name]), name
    assert bool(eager["reward_sum"].abs().sum() > 0)
