"""The comm modes "all" and "random_sample" of the TarMAC-PPO actor on the GPU: mdr_tarmac_gather and mdr_tarmac_gather_backward
against the fp64 restatement of tests/tarmac_gather_ref.py under its derived bounds (every element), the exact recovery of the drawn
sets, the cross-check against the band kernel, refusals, and the whole actor with ``attention="gather"`` - forward, sample, the
captured deployment, the rollout collection and the learner's update."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_ref as ar
from tests import tarmac_gather_ref as gr
from tests import tarmac_ppo_ref as pr
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = gr.load_cases()
MODES = [gr.ALL, gr.RANDOM_SAMPLE]


def _lib():
    import mdr_amd
    return mdr_amd.load_native()


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gather(q, k, v, E, N, c, mode, out, K=None, V=None, seed=gr.SEED, step=gr.STEP, step_dev=None, hop=0, q_off=0):
    """mdr_tarmac_gather on 2-D views (rows = agents; the leading dimension is the view's row stride)."""
    K = q.shape[1] if K is None else K
    V = v.shape[1] if V is None else V
    return _lib().mdr_tarmac_gather(_ptr(q, q_off), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), E, N, K, V, c, mode,
                                    C.c_uint64(seed), C.c_uint64(step), _ptr(step_dev), hop, _ptr(out), out.stride(0), _stream())


def _backward(q, k, v, out, g, E, N, c, mode, dq, dk, dv, ws, seed=gr.SEED, step=gr.STEP, step_dev=None, hop=0):
    K, V = q.shape[1], v.shape[1]
    return _lib().mdr_tarmac_gather_backward(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), E, N, K, V, c, mode,
                                             C.c_uint64(seed), C.c_uint64(step), _ptr(step_dev), hop, _ptr(out), out.stride(0), _ptr(g),
                                             g.stride(0), _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), _ptr(ws),
                                             _stream())


def _ws_bytes(E, N, K, V, c, mode):
    return _lib().mdr_tarmac_gather_backward_workspace_bytes(E, N, K, V, c, mode)


def _dev(a):
    return torch.from_numpy(np.array(a).reshape(a.shape[0] * a.shape[1], -1)).to(DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", gr.GATHER_CASES, ids=str)
def test_forward_holds_the_bound_on_every_element_in_place(shape, mode):
    E, N, c, K, V = shape
    ref = gr.reference(shape, mode)
    q, k, v = (_dev(ref[n]) for n in ("q", "k", "v"))
    out = torch.full((E * N, V), float("nan"), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, E, N, c, mode, out) == 0
    got = out.cpu().numpy().reshape(E, N, V)
    assert np.isfinite(got).all()                                        # every element written, no agent left out
    worst = gr.worst(got, ref["out"], ref["bound"])
    print("%s mode %d: worst |comm - ref| / bound_comm = %.3f" % (shape, mode, worst))
    assert worst <= 1.0
    if N == 1:
        assert torch.equal(out, v)                                       # a softmax over the receiver alone: the value, bit for bit
    # the packed [A][K + K + V] projection buffer read in place, a column block of a wider out written in place, twice the same bits
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    wide = torch.full((E * N, 8 + V + 4), -7.0, dtype=torch.float32, device=DEV)
    assert _gather(qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:], E, N, c, mode, wide[:, 8:8 + V]) == 0
    assert torch.equal(wide[:, 8:8 + V], out)
    assert bool((wide[:, :8] == -7.0).all()) and bool((wide[:, 8 + V:] == -7.0).all())


@pytest.mark.parametrize("mode", MODES)
def test_c_zero_gives_the_value_bit_for_bit(mode):
    E, N, K, V = 3, 20, 8, 16
    q, k, v = (_dev(t) for t in tr.comm_inputs(E, N, K, V))
    out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, E, N, 0, mode, out) == 0
    if mode == gr.RANDOM_SAMPLE:
        assert torch.equal(out, v)
    else:                                                                # "all" ignores nb_comm
        assert not torch.equal(out, v)
        big = torch.empty_like(out)
        assert _gather(q, k, v, E, N, 1000, mode, big) == 0
        assert torch.equal(big, out)


@pytest.mark.parametrize("E,N,c", [(5, 20, 10), (4, 64, 17), (7, 5, 3), (3, 33, 32)])
def test_the_drawn_sets_are_recovered_exactly(E, N, c):
    """q = 0: uniform weights 1 / (c + 1) over the set; one-hot values: out_r holds them at the senders' columns."""
    V = (N + 3) // 4 * 4
    q = torch.zeros((E * N, 8), dtype=torch.float32, device=DEV)
    k = torch.randn((E * N, 8), dtype=torch.float32, device=DEV)
    v = torch.zeros((E, N, V), dtype=torch.float32, device=DEV)
    v[:, torch.arange(N), torch.arange(N)] = 1.0
    v = v.view(E * N, V)
    dev7 = torch.tensor([7], dtype=torch.int32, device=DEV)
    for (seed, step, step_dev), hop in zip(gr.KEYS, (0, 3)):
        out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
        assert _gather(q, k, v, E, N, c, gr.RANDOM_SAMPLE, out, seed=seed, step=step, step_dev=dev7 if step_dev else None, hop=hop) == 0
        got = out.cpu().numpy().reshape(E, N, V)
        want = gr.mask_of(gr.sample_index(E, N, c, seed, step, step_dev or 0, hop), N)
        assert np.array_equal(got[:, :, :N] > 0, want)
        np.testing.assert_allclose(got[:, :, :N][want], 1.0 / (min(c, N - 1) + 1), rtol=2e-7)
        assert not got[:, :, N:].any()
    allout = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, E, N, c, gr.ALL, allout) == 0
    assert bool((allout.view(E, N, V)[:, :, :N] > 0).all())


@pytest.mark.parametrize("shape", [(4, 2, 10, 8, 16), (13, 20, 10, 8, 16), (5, 50, 49, 16, 32), (2, 65, 64, 32, 64)], ids=str)
def test_all_agrees_with_the_band_kernel_at_full_width(shape):
    E, N, _, K, V = shape
    host = tr.comm_inputs(E, N, K, V)
    q, k, v = (_dev(t) for t in host)
    a, b = (torch.empty((E * N, V), dtype=torch.float32, device=DEV) for _ in range(2))
    assert _gather(q, k, v, E, N, 0, gr.ALL, a) == 0
    rc = _lib().mdr_tarmac_comm(_ptr(q), K, _ptr(k), K, _ptr(v), V, E, N, K, V, N - 1, tr.NEIGHBOURS, C.c_float(0.0), C.c_uint64(0), C.c_uint64(0),
                                None, 0, _ptr(b), V, _stream())
    assert rc == 0
    bound = gr.reference(shape, gr.ALL)["bound"] + tr.band_attention(*host, N - 1)[1]
    assert gr.worst(a.cpu().numpy().reshape(E, N, V), b.cpu().numpy().reshape(E, N, V).astype(np.float64), bound) <= 1.0
    # and a full-width sample is the full set: the same senders in another order
    s = torch.empty_like(a)
    assert _gather(q, k, v, E, N, N - 1, gr.RANDOM_SAMPLE, s) == 0
    assert gr.worst(s.cpu().numpy().reshape(E, N, V), a.cpu().numpy().reshape(E, N, V).astype(np.float64), 2 * gr.reference(shape, gr.ALL)["bound"]) <= 1.0


def test_the_draw_does_not_depend_on_the_env_count_or_the_tiling():
    N, c, K, V = 20, 10, 8, 16
    q, k, v = (_dev(t) for t in tr.comm_inputs(13, N, K, V))
    full = torch.empty((13 * N, V), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, 13, N, c, gr.RANDOM_SAMPLE, full) == 0
    part = torch.empty((5 * N, V), dtype=torch.float32, device=DEV)      # 5 envs: another grid, the same agents
    assert _gather(q, k, v, 5, N, c, gr.RANDOM_SAMPLE, part) == 0
    assert torch.equal(part, full[:5 * N])


def test_refusals_launch_nothing():
    from mdr_amd import _native as nat
    E, N = 2, 100
    wide = torch.randn((E * N, 256), dtype=torch.float32, device=DEV)
    out = torch.full((E * N, 80), -7.0, dtype=torch.float32, device=DEV)
    q, k, v = wide[:, :32], wide[:, 32:64], wide[:, 64:144]
    for mode in MODES:
        assert _gather(q, k, v, E, N, 10, mode, out, K=36, V=16) == nat.MDR_ERR_UNSUPPORTED
        assert _gather(q, k, v, E, N, 10, mode, out, K=6, V=16) == nat.MDR_ERR_UNSUPPORTED
        assert _gather(q, k, v, E, N, 10, mode, out, K=8, V=68) == nat.MDR_ERR_UNSUPPORTED
        assert _gather(q, k, v, E, N, 10, mode, out, K=8, V=16, q_off=4) == nat.MDR_ERR_INVALID      # a pointer off 16 bytes
        assert _gather(q, k, v, E, N, 10, mode, out, K=8, V=16, hop=4) == nat.MDR_ERR_INVALID
    assert _gather(q, k, v, E, N, 10, 2, out, K=8, V=16) == nat.MDR_ERR_INVALID                      # an unknown mode
    assert _gather(q, k, v, E, N, 10, -1, out, K=8, V=16) == nat.MDR_ERR_INVALID
    assert _gather(q, k, v, E, N, 65, gr.RANDOM_SAMPLE, out, K=8, V=16) == nat.MDR_ERR_UNSUPPORTED   # c = min(65, 99) > 64
    # an env beyond the LDS limit: 2000 rows of 28 floats are 224,000 bytes
    big = torch.randn((2000, 32), dtype=torch.float32, device=DEV)
    big_out = torch.full((2000, 16), -7.0, dtype=torch.float32, device=DEV)
    for mode in MODES:
        assert _gather(big[:, :8], big[:, 8:16], big[:, 16:], 1, 2000, 10, mode, big_out) == nat.MDR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((big_out == -7.0).all())
    assert _gather(q, k, v, E, N, 64, gr.RANDOM_SAMPLE, out, K=8, V=16) == 0                         # the longest list itself is served
    assert bool((out[:, :16] != -7.0).all()) and bool((out[:, 16:] == -7.0).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [s for s in gr.GATHER_CASES if s[1] <= 256], ids=str)
def test_backward_holds_the_bounds_and_is_bit_stable(shape, mode):
    E, N, c, K, V = shape
    ref = gr.reference(shape, mode)
    q, k, v, g = (_dev(ref[n]) for n in ("q", "k", "v", "g"))
    out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, E, N, c, mode, out) == 0
    nbytes = _ws_bytes(E, N, K, V, c, mode)
    cc = min(c, N - 1)
    assert nbytes == E * N * 16 + ((E * N * cc * 2 + 15) // 16 * 16 if mode == gr.RANDOM_SAMPLE else 0)
    runs = []
    for fill in (0x00, 0xFF):                                            # whatever the workspace held
        ws = torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=DEV)
        grads = [torch.full((E * N, d), float("nan"), dtype=torch.float32, device=DEV) for d in (K, K, V)]
        assert _backward(q, k, v, out, g, E, N, c, mode, *grads, ws) == 0
        runs.append([t.cpu().numpy().reshape(E, N, -1) for t in grads])
    for name, a, b, want, bound in zip(("dq", "dk", "dv"), runs[0], runs[1], ref["grad"], ref["grad_bound"]):
        assert np.isfinite(a).all(), name                                # every element written
        assert np.array_equal(a, b), name
        worst = gr.worst(a, want, bound)
        print("%s mode %d %s: worst / bound = %.3f" % (shape, mode, name, worst))
        assert worst <= 1.0, name
    if cc == 0 and mode == gr.RANDOM_SAMPLE or N == 1:
        assert np.array_equal(runs[0][2], ref["g"]) and not runs[0][0].any() and not runs[0][1].any()


def test_backward_redraws_the_forward_sets_for_another_key():
    shape = (13, 20, 10, 8, 16)
    E, N, c, K, V = shape
    ref = gr.reference(shape, gr.RANDOM_SAMPLE)
    q, k, v, g = (_dev(ref[n]) for n in ("q", "k", "v", "g"))
    seed, step, step_dev = gr.KEYS[1]
    dev7 = torch.tensor([step_dev], dtype=torch.int32, device=DEV)
    out = torch.empty((E * N, V), dtype=torch.float32, device=DEV)
    assert _gather(q, k, v, E, N, c, gr.RANDOM_SAMPLE, out, seed=seed, step=step, step_dev=dev7, hop=2) == 0
    ws = torch.empty(_ws_bytes(E, N, K, V, c, gr.RANDOM_SAMPLE), dtype=torch.uint8, device=DEV)
    grads = [torch.empty((E * N, d), dtype=torch.float32, device=DEV) for d in (K, K, V)]
    assert _backward(q, k, v, out, g, E, N, c, gr.RANDOM_SAMPLE, *grads, ws, seed=seed, step=step, step_dev=dev7, hop=2) == 0
    mask = gr.mask_of(gr.sample_index(E, N, c, seed, step, step_dev, 2), N)
    want, bound = gr.dense_grad(ref["q"], ref["k"], ref["v"], ref["g"], mask), gr.grad_bound(ref["q"], ref["k"], ref["v"], ref["g"], mask)
    for t, w, b, other in zip(grads, want, bound, ref["grad"]):
        got = t.cpu().numpy().reshape(E, N, -1)
        assert gr.worst(got, w, b) <= 1.0
        assert gr.worst(got, other, b) > 1.0                             # and the key matters


def test_backward_refusals_write_nothing():
    from mdr_amd import _native as nat
    K, V = 8, 16
    for E, N, c, mode, want in ((1, 257, 10, gr.ALL, nat.MDR_ERR_UNSUPPORTED), (1, 300, 10, gr.RANDOM_SAMPLE, nat.MDR_ERR_UNSUPPORTED),
                                (2, 100, 65, gr.RANDOM_SAMPLE, nat.MDR_ERR_UNSUPPORTED), (2, 100, 10, 2, nat.MDR_ERR_INVALID)):
        A = E * N
        q, k, v, g, out = (torch.randn((A, d), dtype=torch.float32, device=DEV) for d in (K, K, V, V, V))
        grads = [torch.full((A, d), -7.0, dtype=torch.float32, device=DEV) for d in (K, K, V)]
        ws = torch.zeros(A * 16 + A * 64 * 2 + 16, dtype=torch.uint8, device=DEV)
        assert _backward(q, k, v, out, g, E, N, c, mode, *grads, ws) == want
        assert _backward(q, k, v, out, g, E, min(N, 256), min(c, 64), gr.ALL if mode == 2 else mode, *grads, None) == nat.MDR_ERR_INVALID      # no workspace
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in grads) and not bool(ws.any())
    assert _ws_bytes(2, 20, 8, 16, 10, 2) == -1 and _ws_bytes(2, 20, 36, 16, 10, 0) == -1 and _ws_bytes(2, 0, 8, 16, 10, 0) == -1


def test_gather_attention_autograd_matches_the_kernels_and_dense_autograd():
    from mdr_amd.tarmac import gather_attention
    shape = (13, 20, 10, 8, 16)
    E, N, c, K, V = shape
    for mode in MODES:
        ref = gr.reference(shape, mode)
        # column blocks of one packed buffer: read in place through their row stride
        qkv = torch.cat([torch.from_numpy(np.array(ref[n])) for n in ("q", "k", "v")], dim=2).to(DEV).requires_grad_(True)
        out = gather_attention(qkv[:, :, :K], qkv[:, :, K:2 * K], qkv[:, :, 2 * K:], c, gr.MODE_NAMES[mode], seed=gr.SEED, step=gr.STEP)
        assert gr.worst(out.detach().cpu().numpy(), ref["out"], ref["bound"]) <= 1.0
        (out * torch.from_numpy(np.array(ref["g"])).to(DEV)).sum().backward()
        got = qkv.grad.cpu().numpy()
        for part, want, bound in zip((got[:, :, :K], got[:, :, K:2 * K], got[:, :, 2 * K:]), ref["grad"], ref["grad_bound"]):
            assert gr.worst(part, want, bound) <= 1.0
    with pytest.raises(ValueError):
        gather_attention(qkv[:, :, :K], qkv[:, :, K:2 * K], qkv[:, :, 2 * K:], c, "neighbours")


# ---------------------------------------------------------------------------------------------------------------- the whole actor

def _masks(case, E, seed, step, step_dev=0):
    """bool [hops, E, N, N]: what the kernels draw for (seed, step), or ones."""
    return torch.from_numpy(np.stack([gr.mask_of(gr.index_of(case["mode"], E, case["N"], case["c"], seed, step, step_dev, hop), case["N"])
                                      for hop in range(case["hops"])]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_cases_through_the_gather_path(name):
    case = CASES[name]
    actor = gr.make_actor(case, "gather").to(DEV)
    obs = torch.from_numpy(case["obs"]).to(DEV)
    seed, step = 9, 4
    with torch.no_grad():
        p = actor(obs, seed=seed, step=step)
    assert p.shape == case["probs"].shape and p.dtype == torch.float32
    if case["mode"] == gr.ALL:
        want = case["probs"]                                             # the reference's own fp64 values
    else:                                                                # the fp64 dense path, fed the masks of sample_index
        with torch.no_grad():
            want = gr.make_actor(case, "dense", torch.float64)(torch.from_numpy(case["obs"]).double(), mask=_masks(case, 4, seed, step)).numpy()
        assert ar.contract_ratio(p.cpu().numpy(), case["probs"], False).max() > 1.0      # not the reference's np.random masks
    ratio = ar.contract_ratio(p.cpu().numpy(), want, False).max()
    print("%s: %.3f of the probability contract" % (name, ratio))
    assert ratio <= 1.0
    action, a_prob, probs = actor.sample(obs, seed=seed, step=step, want_probs=True)
    assert torch.equal(probs.view_as(p), p)                              # the same GEMMs and kernels again
    u = ar.draw_u(np.arange(action.numel()), seed, step)
    assert np.array_equal(action.cpu().numpy(), ar.expected_action(u, probs[:, 0].cpu().numpy(), False, None))
    # the differentiable chain: the same probabilities within the contract, gradients in every parameter the hops reach
    pd = actor(obs, seed=seed, step=step, differentiable=True)
    assert pd.requires_grad and ar.contract_ratio(pd.detach().cpu().numpy(), want, False).max() <= 1.0
    pd[:, :, 0].sum().backward()
    for n, prm in actor.named_parameters():
        if case["hops"] > 1 or "msg_state2state" not in n:
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and bool(prm.grad.abs().sum() > 0), n
    # the dense path on the device with the same masks
    with torch.no_grad():
        pm = gr.make_actor(case, "dense").to(DEV)(obs, mask=_masks(case, 4, seed, step).to(DEV))
    assert ar.contract_ratio(pm.cpu().numpy(), want, False).max() <= 1.0


def _env(E, N, **kw):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=3, **kw)
    env.reset(episode=0)
    return env


def _actor(F, N, mode, attention="gather"):
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    torch.manual_seed(11)
    actor, critic = TarMACActor(F, comm_mode=mode, attention=attention), TarMACCritic(N, F)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return actor.to(DEV), critic.to(DEV)


@pytest.mark.parametrize("mode", ["all", "random_sample"])
def test_captured_deployment_equals_the_eager_one(mode):
    import mdr_amd
    from mdr_amd.rollout import deploy_policy
    E, N, T = 2, 20, 8
    cfg = _env(1, N).config
    envs = [mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=2, table_steps=16, graph_mode=True) for _ in range(2)]
    for e in envs:
        e.reset(episode=0)
    actor, _ = _actor(envs[0].obs_vector_length(), N, mode)
    eager = deploy_policy(envs[0], actor, T, seed=7, use_graph=False)
    graph = deploy_policy(envs[1], actor, T, seed=7, use_graph=True)
    for name in ("reward_sum", "sq_temp_error_sum", "sq_signal_error_sum"):
        assert torch.equal(eager[name], graph[name]), name
    assert bool(eager["reward_sum"].abs().sum() > 0)


@pytest.mark.parametrize("mode", ["all", "random_sample"])
def test_collect_tarmac_rollout_stores_what_forward_reproduces(mode):
    from mdr_amd.rollout import collect_tarmac_rollout, deploy_policy
    E, N, T, seed = 3, 20, 4, 5
    env = _env(E, N)
    F = env.obs_vector_length()
    actor, critic = _actor(F, N, mode)
    step0 = env.steps_taken
    ro = collect_tarmac_rollout(env, actor, T, gamma=0.9, critic=critic, seed=seed)
    A = E * N
    assert ro["state"].shape == (T + 1, A, F) and ro["a_prob"].shape == (T, A) and env.steps_taken == step0 + T
    agents = torch.arange(A, device=DEV)
    for t in range(T):
        with torch.no_grad():
            p = actor(ro["state"][t].view(E, N, F), seed=seed, step=step0 + t).view(A, 2)
        assert torch.equal(ro["a_prob"][t], p[agents, ro["action"][t]])
        u = ar.draw_u(np.arange(A), seed, step0 + t)
        assert np.array_equal(ro["action"][t].cpu().numpy(), ar.expected_action(u, p[:, 0].cpu().numpy(), False, None))
    if mode == "random_sample":                                          # the key matters: another step, other senders
        with torch.no_grad():
            assert not torch.equal(actor(ro["state"][0].view(E, N, F), seed=seed, step=step0 + 1).view(A, 2), p)
    assert 0.05 < ro["action"].float().mean().item() < 0.95
    out = deploy_policy(_env(E, N), actor, T, seed=seed)                 # eager deployment: the same actions as the collection
    torch.testing.assert_close(out["reward_sum"], ro["reward"].view(T, E, N).sum(dim=0))


@pytest.mark.parametrize("mode", ["all", "random_sample"])
def test_learner_update_against_fp64_dense_autograd(mode):
    """One minibatch of all T E = 8 env-steps through TarMACPPOLearner (torch backend: forward(differentiable=True), i.e.
    gather_attention): every parameter's gradient within 4 x the distance of float32 dense autograd from fp64 dense autograd on the
    same masks, in relative L2 (the measured ratios: profiles/tarmac_gather_README.md)."""
    from mdr_amd import tarmac_ppo as tp
    from mdr_amd.rollout import collect_tarmac_rollout
    E, N, T, seed, clip = 2, 20, 4, 5, 0.2
    env = _env(E, N)
    F = env.obs_vector_length()
    actor, critic = _actor(F, N, mode)
    ro = collect_tarmac_rollout(env, actor, T, gamma=0.9, critic=critic, seed=seed)
    kw = dict(lr_actor=1.0, lr_critic=1e-3, clip_param=clip, max_grad_norm=1e30, ppo_update_time=1, batch_size=T * E, optimizer=torch.optim.SGD)
    a, c = copy.deepcopy(actor), copy.deepcopy(critic)
    learner = tp.TarMACPPOLearner(a, c, backend="auto", **kw)
    assert not learner.uses_kernels(T * E) and not tp.supported(a)       # the fused update kernels keep refusing these modes
    with pytest.raises(ValueError):
        tp.TarMACPPOLearner(copy.deepcopy(actor), copy.deepcopy(critic), backend="hip", **kw)
    index = learner.minibatches(T * E, seed, 0)[0]
    assert index.numel() == T * E
    state = ro["state"][:T].reshape(T * E, N, F)
    action, old, target = (ro[k].reshape(T * E, N) for k in ("action", "a_prob", "return"))
    with torch.no_grad():
        advantage = target[index] - critic(state[index])
    a_loss, c_loss = learner.step_minibatch(state, action, old, target, index, seed=seed)
    assert bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
    grads = {"gather": {n: p.grad.detach().double().cpu().numpy() for n, p in a.named_parameters() if p.grad is not None}}
    # minibatch row i stands for env i in the key, the learner's step counter was 0
    case = dict(mode=gr.ALL if mode == "all" else gr.RANDOM_SAMPLE, N=N, c=actor.number_agents_comm, hops=1)
    masks = _masks(case, T * E, seed, 0)
    for name, dt in (("dense32", torch.float32), ("dense64", torch.float64)):
        d = copy.deepcopy(actor).cpu().to(dt)
        d.attention = "dense"
        prob = d(state[index].cpu().to(dt), mask=masks).gather(2, action[index].cpu().unsqueeze(2)).squeeze(2)
        ratio = prob / old[index].cpu().to(dt)
        adv = advantage.cpu().to(dt)
        loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
        loss.backward()
        grads[name] = {n: p.grad.detach().double().numpy() for n, p in d.named_parameters() if p.grad is not None}
    assert set(grads["gather"]) == set(grads["dense64"]) and len(grads["dense64"]) == 20
    # tarmac_ppo_ref.rel_l2: ||got - ref|| / ||ref|| per tensor; hidden2key's last bias shifts every score of a receiver alike, its
    # gradient vanishes exactly, so its error (and its yardstick) is taken relative to the largest gradient norm of the case
    err, yard = pr.rel_l2(grads["gather"], grads["dense64"]), pr.rel_l2(grads["dense32"], grads["dense64"])
    for n in sorted(err):
        print("%-14s %-34s gather %.3e  float32 dense %.3e  ratio %.2f" % (mode, n, err[n], yard[n], err[n] / yard[n]))
    assert abs(float(a_loss) - float(loss.detach())) <= 1e-5 * max(1.0, abs(float(loss.detach())))
    # A relative error needs a gradient to be relative to.  The one tensor whose fp64 gradient vanishes is held to what the existing
    # learner tests allow such a tensor (tarmac_ppo_ref.FLOOR = 2^-20 = 16 u of the case's largest gradient norm): what either
    # evaluation leaves there is the residue of sum_s ds_rs = 0, taken through different formulas (delta = g . out against
    # rowsum(P dP)), not a fraction of one another.  Every other tensor: 4 x the yardstick, nothing else.
    top = max(np.linalg.norm(g) for g in grads["dense64"].values())
    vanishing = {n for n, g in grads["dense64"].items() if np.linalg.norm(g) <= 1e-6 * top}
    assert vanishing == {"comm.hidden2key.2.bias"}
    for n in err:
        assert err[n] <= (max(4.0 * yard[n], pr.FLOOR) if n in vanishing else 4.0 * yard[n]), (n, err[n], yard[n])
    # a whole update with Adam: finite, and the parameters moved
    kw.update(lr_actor=1e-2, lr_critic=1e-2, optimizer=torch.optim.Adam, max_grad_norm=0.5, ppo_update_time=2, batch_size=4)
    a, c = copy.deepcopy(actor), copy.deepcopy(critic)
    a_loss, c_loss, count = tp.TarMACPPOLearner(a, c, backend="auto", **kw).update(ro, seed=1)
    assert count == 2 * 2 and bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
    assert all(bool(torch.isfinite(p).all()) for p in list(a.parameters()) + list(c.parameters()))
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), actor.parameters()))
