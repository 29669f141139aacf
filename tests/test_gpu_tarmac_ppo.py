"""TarMAC-PPO's update step on the GPU: mdr_tarmac_ppo_actor_grad against the reference's formula in float64 (tests/tarmac_ppo_ref.py)
under the contract of test_gpu_tarmac_grad.py::test_differentiable_forward_end_to_end - per parameter tensor, relative L2 error <=
max(8 x the error of the float32 dense path on the CPU, 2^-20) -, loss and ratios within actor_ref.CONTRACT[False]; tiling, index,
determinism, dead senders, refusals, and TarMACPPOLearner's hip backend against its torch backend.

Largest error / max(yardstick, floor / 8) per case on the MI355X (the contract allows 8; forward(differentiable=True) measured up to
4.05, profiles/tarmac_grad_README.md): see profiles/tarmac_ppo_README.md."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import actor_ref as ar
from tests import tarmac_ppo_ref as pr
from tests import tarmac_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = tr.load_cases()


def _tp():
    from mdr_amd import tarmac_ppo
    return tarmac_ppo


def _run(d, actor=None, index=None, state=None, adv=None, max_workgroups=0, seed=0, step=0):
    """-> (loss float64, ratio [B, N] float64 numpy, {name: gradient float64 numpy}, actor on the device)."""
    actor = copy.deepcopy(d["actor"]).to(DEV) if actor is None else actor
    actor.zero_grad(set_to_none=True)
    state = d["state"].to(DEV) if state is None else state
    adv = d["adv"] if adv is None else adv
    loss, ratio = _tp().actor_loss_backward(actor, state, d["action"].to(DEV), d["old_prob"].to(DEV), adv.to(DEV), pr.CLIP, index=index,
                                            seed=seed, step=step, want_ratio=True, max_workgroups=max_workgroups)
    grads = {n: p.grad.detach().double().cpu().numpy() for n, p in actor.named_parameters() if p.grad is not None}
    return float(loss.double().cpu()), ratio.double().cpu().numpy(), grads, actor


def _hold(label, d, loss, ratio, grads, yard=None):
    ref = d if yard is None else dict(d, yard=yard)
    score, worst, err = pr.holds(grads, ref)
    print("%s: %d tensors, largest relative L2 error %.3e (yardstick's largest %.3e); largest error / max(yardstick, floor / factor) = %.3f at "
          "%s (error %.3e, yardstick %.3e); loss %.9g (fp64 %.9g)" % (label, len(err), max(err.values()), max(ref["yard"].values()), score, worst,
                                                                      err[worst], ref["yard"][worst], loss, d["loss"]))
    for n in err:
        assert err[n] <= max(pr.FACTOR * ref["yard"][n], pr.FLOOR), (label, n, err[n], ref["yard"][n])
    assert ar.contract_ratio(np.array([loss]), np.array([d["loss"]]), False).max() <= 1.0, (loss, d["loss"])
    assert ar.contract_ratio(ratio, d["ratio"], False).max() <= 1.0
    return score


@pytest.mark.parametrize("name", pr.ONE_HOP)
def test_recorded_one_hop_cases(name):
    d = pr.recorded(name)
    loss, ratio, grads, actor = _run(d)
    _hold(name, d, loss, ratio, grads)
    if d["case"]["with_comm"]:
        assert all(p.grad is None for p in actor.comm.msg_state2state.parameters())      # not reached, not touched
    if d["case"]["with_comm"] and d["case"]["mode"] == tr.NONE:                           # exact zeros, as the attention's backward documents
        assert all(not g.any() for n, g in grads.items() if n.startswith("comm."))


@pytest.mark.parametrize("name", sorted(pr.SYNTHETIC))
def test_tiling_band_and_a_second_pass_of_the_grid(name):
    d = pr.synthetic(name)
    loss, ratio, grads, _ = _run(d, max_workgroups=d["max_workgroups"])
    _hold(name, d, loss, ratio, grads)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_index_and_padded_rows_are_the_gathered_copy_bit_for_bit():
    d = pr.recorded("f22_n20_c10")
    index = torch.tensor([3, 0, 3, 1, 2], dtype=torch.int64)
    adv = d["adv"][index].contiguous()
    loss_i, ratio_i, grads_i, _ = _run(d, index=index.to(DEV), adv=adv)
    gathered = dict(d, state=d["state"][index].contiguous(), action=d["action"][index].contiguous(), old_prob=d["old_prob"][index].contiguous())
    loss_g, ratio_g, grads_g, _ = _run(gathered, adv=adv)
    assert loss_i == loss_g and np.array_equal(ratio_i, ratio_g)
    for n in grads_g:
        assert np.array_equal(grads_i[n], grads_g[n]), n
    # a padded row stride
    M, N, F = d["state"].shape
    wide = torch.full((M, N, F + 5), float("nan"), device=DEV)
    wide[:, :, :F] = d["state"].to(DEV)
    loss_p, ratio_p, grads_p, _ = _run(d, state=wide[:, :, :F])
    loss_c, ratio_c, grads_c, _ = _run(d)
    assert loss_p == loss_c and np.array_equal(ratio_p, ratio_c)
    for n in grads_c:
        assert np.array_equal(grads_p[n], grads_c[n]), n


CANARY = 12345.0


def _direct(actor, state, action, old, adv, B, N, desc=None, workspace="own", max_workgroups=0, seed=0, step=0):
    """The C call on NaN-filled outputs between canaries -> (rc, grad, loss, ratio: the bracketed buffers, the workspace)."""
    tp, lib = _tp(), nat.load()
    desc = tp._desc(actor) if desc is None else desc
    G = sum(p.numel() for p in tp._params(actor))
    out = {"grad": G, "loss": 1, "ratio": max(B * N, 1)}
    bufs = {}
    for k, n in out.items():
        b = torch.full((n + 8,), float("nan"), device=DEV)      # 4 floats of canary on either side: the payload stays 16-byte aligned
        b[:4] = CANARY
        b[-4:] = CANARY
        bufs[k] = b
    ws = None
    if workspace == "own":
        nbytes = lib.mdr_tarmac_ppo_workspace_bytes(C.byref(tp._desc(actor)), B, N, max_workgroups)
        ws = torch.full((max(nbytes, 16) // 4 + 4,), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.mdr_tarmac_ppo_actor_grad(C.byref(desc), C.c_void_p(state.data_ptr()), state.shape[-1], None, B, N, C.c_void_p(action.data_ptr()),
                                           C.c_void_p(old.data_ptr()), C.c_void_p(adv.data_ptr()), C.c_float(pr.CLIP), C.c_uint64(seed), C.c_uint64(step),
                                           max_workgroups, C.c_void_p(ws.data_ptr()) if ws is not None else None,
                                           C.c_void_p(bufs["grad"].data_ptr() + 16), C.c_void_p(bufs["loss"].data_ptr() + 16),
                                           C.c_void_p(bufs["ratio"].data_ptr() + 16), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bufs["grad"], bufs["loss"], bufs["ratio"], ws


def _canaries_intact(*bufs):
    return all(bool((b[:4] == CANARY).all()) and bool((b[-4:] == CANARY).all()) for b in bufs)


@pytest.mark.parametrize("name", ["f22_n20_c10", "f22_n20_nocomm"])
def test_every_float_is_written_and_two_calls_give_the_same_bits(name):
    d = pr.recorded(name)
    actor = copy.deepcopy(d["actor"]).to(DEV)
    state, action, old, adv = (d[k].to(DEV) for k in ("state", "action", "old_prob", "adv"))
    B, N = adv.shape
    rc, grad, loss, ratio, _ = _direct(actor, state, action, old, adv, B, N)
    assert rc == 0
    assert _canaries_intact(grad, loss, ratio)
    for b in (grad, loss, ratio):
        assert bool(torch.isfinite(b[4:-4]).all())
    rc2, grad2, loss2, ratio2, _ = _direct(actor, state, action, old, adv, B, N)
    assert rc2 == 0
    for a, b in ((grad, grad2), (loss, loss2), (ratio, ratio2)):
        assert torch.equal(_bits(a), _bits(b))
    # another grid gives another summation order, never another value beyond rounding; the same grid the same bits
    rc3, grad3, _, _, _ = _direct(actor, state, action, old, adv, B, N, max_workgroups=1)
    rc4, grad4, _, _, _ = _direct(actor, state, action, old, adv, B, N, max_workgroups=1)
    assert rc3 == 0 and rc4 == 0 and torch.equal(_bits(grad3), _bits(grad4))
    torch.testing.assert_close(grad3[4:-4], grad[4:-4], rtol=1e-4, atol=1e-7)
    # no rows: zeros in grad and loss, nothing else touched
    rc0, grad0, loss0, ratio0, _ = _direct(actor, state, action, old, adv, 0, N)
    assert rc0 == 0 and _canaries_intact(grad0, loss0, ratio0)
    assert not bool(grad0[4:-4].any()) and float(loss0[4]) == 0.0 and bool(torch.isnan(ratio0[4:-4]).all())


@pytest.mark.parametrize("step", pr.DEFECT_STEPS)
def test_dead_senders_are_those_of_the_differentiable_forward(step):
    d = pr.recorded("f22_n20_c10", step)
    seed = pr.DEFECT_SEED
    index = torch.tensor([2, 0, 1, 3], dtype=torch.int64)
    # the yardstick: the band path under autograd, float32 on the GPU, against fp64 with the mask of tarmac_ref.dead_mask
    band = tr.make_actor(d["case"], attention="band", defect_prob=pr.DEFECT_PROB).to(DEV)
    inv = torch.argsort(index)
    state = d["state"][inv].contiguous().to(DEV)          # state[index] is the case's observations: row i stands for env i
    prob = band(state[index.to(DEV)], seed=seed, step=step, differentiable=True).gather(2, d["action"].to(DEV).unsqueeze(2)).squeeze(2)
    ratio = prob / d["old_prob"].to(DEV)
    adv = d["adv"].to(DEV)
    (-torch.min(ratio * adv, torch.clamp(ratio, 1 - pr.CLIP, 1 + pr.CLIP) * adv).mean()).backward()
    yard = pr.rel_l2({n: p.grad.double().cpu().numpy() for n, p in band.named_parameters() if p.grad is not None}, d["grad"])
    moved = dict(d, action=d["action"][inv].contiguous(), old_prob=d["old_prob"][inv].contiguous())
    actor = tr.make_actor(d["case"], attention="band", defect_prob=pr.DEFECT_PROB).to(DEV)
    loss, ratio_k, grads, _ = _run(moved, actor=actor, index=index.to(DEV), state=state, seed=seed, step=step)
    _hold("defects step %#x" % step, d, loss, ratio_k, grads, yard=yard)
    # another key draws another mask: the gradient leaves the contract
    _, _, other, _ = _run(moved, actor=actor, index=index.to(DEV), state=state, seed=seed, step=step + 1)
    err = pr.rel_l2(other, d["grad"])
    assert max(err[n] / max(pr.FACTOR * yard[n], pr.FLOOR) for n in err) > 10.0


def test_refusals_leave_every_output_untouched():
    tp = _tp()
    d = pr.recorded("f22_n20_c10")
    actor = copy.deepcopy(d["actor"]).to(DEV)
    state, action, old, adv = (d[k].to(DEV) for k in ("state", "action", "old_prob", "adv"))
    B, N = adv.shape

    def refused(expect, **kw):
        rc, grad, loss, ratio, ws = _direct(actor, state, action, old, adv, B, N, **kw)
        assert rc == expect, (rc, kw)
        assert _canaries_intact(grad, loss, ratio)
        assert all(bool(torch.isnan(b[4:-4]).all()) for b in (grad, loss, ratio))
        assert ws is None or bool(torch.isnan(ws).all())

    def desc(**fields):
        s = tp._desc(actor)
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    refused(nat.MDR_ERR_UNSUPPORTED, desc=desc(num_hops=2))
    refused(nat.MDR_ERR_UNSUPPORTED, desc=desc(hidden=68))
    refused(nat.MDR_ERR_UNSUPPORTED, desc=desc(num_key=20))
    refused(nat.MDR_ERR_UNSUPPORTED, desc=desc(mode=2))
    refused(nat.MDR_ERR_INVALID, workspace=None)
    refused(nat.MDR_ERR_INVALID, desc=desc(struct_size=8))
    refused(nat.MDR_ERR_INVALID, desc=desc(head_w0=None))
    two_hops = tr.make_actor(CASES["f51_n50_c10_hops2"], attention="band").to(DEV)
    assert not tp.supported(two_hops)
    with pytest.raises(ValueError, match="one hop"):
        tp.actor_loss_backward(two_hops, torch.zeros((2, 50, 51), device=DEV), torch.zeros((2, 50), dtype=torch.int64, device=DEV),
                               torch.ones((2, 50), device=DEV), torch.ones((2, 50), device=DEV))


def _env(E, N):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=3)
    env.reset(episode=0)
    return env


def test_learner_hip_backend_against_torch_backend():
    from mdr_amd.rollout import collect_tarmac_rollout
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    tp = _tp()
    E, N, T = 8, 20, 6
    env = _env(E, N)
    F = env.obs_vector_length()
    torch.manual_seed(11)
    actor, critic = TarMACActor(F).to(DEV), TarMACCritic(N, F).to(DEV)
    ro = collect_tarmac_rollout(env, actor, T, gamma=0.9, critic=critic, seed=5)
    kw = dict(clip_param=0.2, max_grad_norm=0.5, ppo_update_time=2, batch_size=16)
    before = {n: p.detach().double().cpu().numpy().copy() for n, p in actor.named_parameters()}
    # one minibatch under plain SGD with lr = 1 (the update is minus the clipped gradient): hip, torch on the GPU, and torch in float64
    # on the CPU.  The update is p_after - p_before, which a float32 parameter holds to half an ulp of ITSELF - for the key and query
    # projections, whose gradients are 1e-4 of the others', that rounding is the whole error of either backend - so the clipped
    # gradient the optimiser consumed (SGD leaves it in .grad) is held to the contract as well.
    learners = {}
    for name, dev, dt, backend, attention in (("hip", DEV, torch.float32, "hip", "auto"), ("torch", DEV, torch.float32, "torch", "auto"),
                                              ("fp64", "cpu", torch.float64, "torch", "dense")):
        a, c = copy.deepcopy(actor).to(dev).to(dt), copy.deepcopy(critic).to(dev).to(dt)
        a.attention = attention
        learners[name] = tp.TarMACPPOLearner(a, c, lr_actor=1.0, lr_critic=1e-3, backend=backend, optimizer=torch.optim.SGD, **kw)
    assert learners["hip"].uses_kernels(1) and not learners["torch"].uses_kernels(16)
    index = learners["hip"].minibatches(T * E, 0, 0)[0]
    delta, clipped = {}, {}
    for name, learner in learners.items():
        dev, dt = next(learner.actor.parameters()).device, next(learner.actor.parameters()).dtype
        state = ro["state"][:T].reshape(T * E, N, F).to(dev).to(dt)
        action, old, target = (ro[k].reshape(T * E, N).to(dev) for k in ("action", "a_prob", "return"))
        a_loss, c_loss = learner.step_minibatch(state, action, old.to(dt), target.to(dt), index.to(dev))
        assert bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
        reached = [(n, p) for n, p in learner.actor.named_parameters() if "msg_state2state" not in n]
        delta[name] = {n: p.detach().double().cpu().numpy() - before[n] for n, p in reached}
        clipped[name] = {n: p.grad.detach().double().cpu().numpy() for n, p in reached}
    for what, got in (("update", delta), ("clipped gradient", clipped)):
        yard, err = pr.rel_l2(got["torch"], got["fp64"]), pr.rel_l2(got["hip"], got["fp64"])
        worst = max(err, key=lambda n: err[n] / max(yard[n], pr.FLOOR / pr.FACTOR))
        print("one minibatch, %s: largest relative L2 error hip %.3e, torch %.3e; largest hip / max(torch, floor / factor) = %.3f at %s "
              "(hip %.3e, torch %.3e)" % (what, max(err.values()), max(yard.values()), err[worst] / max(yard[worst], pr.FLOOR / pr.FACTOR), worst,
                                          err[worst], yard[worst]))
        for n in err:
            assert err[n] <= max(pr.FACTOR * yard[n], pr.FLOOR), (what, n, err[n], yard[n])
    kw.update(lr_actor=1e-2, lr_critic=1e-2)
    hip = learners["hip"].actor
    flat = hip._mdr_flat_grad
    for p in tp._params(hip):
        assert p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    assert all(p.grad is None for p in hip.comm.msg_state2state.parameters())
    # a full update with Adam: finite losses, no NaN
    a, c = copy.deepcopy(actor), copy.deepcopy(critic)
    full = tp.TarMACPPOLearner(a, c, backend="auto", **kw)
    assert full.uses_kernels(16)
    a_loss, c_loss, count = full.update(ro, seed=1)
    assert count == 2 * 3 and bool(torch.isfinite(a_loss)) and bool(torch.isfinite(c_loss))
    assert all(bool(torch.isfinite(p).all()) for p in list(a.parameters()) + list(c.parameters()))
    assert any(not torch.equal(p, q) for p, q in zip(a.parameters(), actor.parameters()))
    # two hops: auto falls back, hip refuses
    two = TarMACActor(F, num_hops=2).to(DEV)
    assert not tp.TarMACPPOLearner(two, copy.deepcopy(critic), backend="auto", **kw).uses_kernels(256)
    with pytest.raises(ValueError, match="one hop"):
        tp.TarMACPPOLearner(two, copy.deepcopy(critic), backend="hip", **kw)
