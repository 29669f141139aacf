"""The batched form of MADDPG's unshared update (mdr_maddpg_target_all, mdr_maddpg_critic_grad_all, mdr_maddpg_actor_grad_all,
mdr_adam_step_nets, ``MADDPGLearner(agent_steps="batched")``) against the sequential form, bit for bit: the contract of the batched
form is the BITS of the per-agent calls, so every comparison here is ``torch.equal`` and there is no tolerance to choose.

Numerical correctness - against torch autograd, the fp64 restatements and the reference's own ``update()`` - is pinned for the
sequential hip path in tests/test_gpu_maddpg_agents_learner.py and tests/test_gpu_learner_golden.py; bit-equality with that path
carries it over to the batched one.

Shapes (N, F, H, B), the smallest that reach every branch: (3, 51, 100, 17) - tests/test_gpu_maddpg_learner.py's own, a partial
second tile per agent, H no multiple of 16; (2, 5, 20, 16) - one exact tile, one 16-unit block and a ragged one; (1, 51, 100, 17);
(32, 8, 16, 3) - the last slot of the tables, J = 320; and once the reference's (20, 51, 256, 64)."""
import ctypes as C

import pytest
import torch

from tests import maddpg_grad_ref as R
from tests.test_gpu_maddpg_agents_learner import _case_nets
from tests.test_gpu_maddpg_learner import B, DEV, F_LEN, H, LR_A, LR_C, N, SOFT_TAU, TAU, _dev

pytestmark = pytest.mark.gpu

SHAPES = [(3, 51, 100, 17), (2, 5, 20, 16), (1, 51, 100, 17), (32, 8, 16, 3), (20, 51, 256, 64)]
PAD = 64      # canary bytes on either side of an output


def _random_case(n, f, h, b, seed=3):
    """Distinct nets per agent (actor, critic, target actor, target critic), a buffer of env-steps, one minibatch and its noise per
    agent in the layouts mdr_maddpg_draws writes."""
    from mdr_amd.maddpg import DDPGNetworkMLP
    torch.manual_seed(seed)
    nets = [[DDPGNetworkMLP(f, 2, h).to(DEV), DDPGNetworkMLP(n * (f + 2), 1, h).to(DEV), DDPGNetworkMLP(f, 2, h).to(DEV),
             DDPGNetworkMLP(n * (f + 2), 1, h).to(DEV)] for _ in range(n)]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    m = b + 9
    data = dict(state=torch.randn((m, n, f), generator=gen, device=DEV), next_state=torch.randn((m, n, f), generator=gen, device=DEV),
                action=torch.randint(0, 2, (m, n), generator=gen, device=DEV), reward=torch.randn((m, n), generator=gen, device=DEV))
    index = torch.stack([torch.randperm(m, generator=gen, device=DEV)[:b] for _ in range(n)])
    noise = -torch.empty((n, b, n + 1, 2), device=DEV).exponential_(generator=gen).log()
    return nets, data, index, noise[:, :, :n].contiguous(), noise[:, :, n].contiguous()


def _canary(shape, dtype):
    """(the whole buffer of 0xFF bytes, the output inside it)."""
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((PAD + nbytes + PAD,), 0xFF, dtype=torch.uint8, device=DEV)
    return whole, whole[PAD:PAD + nbytes].view(dtype).view(shape)


def _intact(whole):
    return bool((whole[:PAD] == 0xFF).all()) and bool((whole[-PAD:] == 0xFF).all())


def _grad(module):
    return module._mdr_flat_grad.clone()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_F%d_H%d_B%d" % s)
def test_every_all_call_writes_the_bits_of_the_single_agent_calls(shape):
    from mdr_amd import _learner as L
    from mdr_amd import _native as nat
    from mdr_amd import maddpg as M
    n, f, h, b = shape
    nets, data, index, noise_t, noise_a = _random_case(n, f, h, b)
    actors, critics, tgt_actors, tgt_critics = ([x[k] for x in nets] for k in range(4))
    gamma, tau = 0.99, 0.5
    # ---- the N single-agent calls
    want = dict(y=[], next_q=[], next_action=[], c_loss=[], c_q=[], c_grad=[], a_loss=[], a_q=[], a_logits=[], a_grad=[])
    for a in range(n):
        y, next_q, next_action = M.maddpg_target(tgt_actors, tgt_critics[a], data["next_state"], data["reward"], a, noise_t[a], tau, gamma,
                                                 index=index[a])
        loss, q = M.joint_q_loss_backward(actors[a], critics[a], data["state"], data["action"], y, index=index[a], want_q=True)
        want["y"].append(y), want["next_q"].append(next_q), want["next_action"].append(next_action)
        want["c_loss"].append(loss.clone()), want["c_q"].append(q), want["c_grad"].append(_grad(critics[a]))
        loss, q, logits = M.actor_loss_backward(actors[a], critics[a], data["state"], data["action"], a, noise_a[a], tau, M.PSE, index=index[a],
                                                want_q=True)
        want["a_loss"].append(loss.clone()), want["a_q"].append(q), want["a_logits"].append(logits), want["a_grad"].append(_grad(actors[a]))
    want = {k: torch.stack(v) for k, v in want.items()}
    # ---- the three calls over all agents, at the library's grid and with one workgroup
    lib = nat.load()
    adescs, cdescs, tadescs, tcdescs = (L.mlp_descs([L.fc_layers(m) for m in group]) for group in (actors, critics, tgt_actors, tgt_critics))
    a_floats, c_floats, _ = M._sizes(adescs[0], cdescs[0], n, b)
    nbytes = int(lib.mdr_maddpg_workspace_bytes_all(C.byref(adescs[0]), C.byref(cdescs[0]), n, b, 0))
    assert nbytes > 0
    ld = n * f
    for mw in (0, 1):
        out = {k: _canary(v.shape, v.dtype) for k, v in want.items()}
        ws, _ = _canary((nbytes,), torch.uint8)      # 0xFF bytes: NaNs wherever the kernels read what they did not write
        ws = ws[PAD:PAD + nbytes]
        with torch.cuda.device(DEV):
            st = L.stream(torch.device(DEV))
            M._target_all_launch(tadescs, tcdescs, data["next_state"], ld, data["reward"], index, b, n, noise_t, out["y"][1], out["next_q"][1],
                                 out["next_action"][1], st, tau, gamma, mw)
            M._critic_all_launch(cdescs, data["state"], ld, data["action"], index, b, n, out["y"][1], ws, out["c_grad"][1], out["c_loss"][1],
                                 out["c_q"][1], st, mw)
            M._actor_all_launch(adescs, cdescs, data["state"], ld, data["action"], index, b, n, noise_a, ws, out["a_grad"][1], out["a_loss"][1],
                                out["a_q"][1], out["a_logits"][1], st, tau, M.PSE, mw)
        for k, v in want.items():
            assert out[k][1].shape == v.shape and (a_floats, c_floats) == (want["a_grad"].shape[1], want["c_grad"].shape[1])
            for a in range(n):
                assert torch.equal(out[k][1][a], v[a]), (k, a, mw)
            assert _intact(out[k][0]), (k, mw)
        assert bool(torch.isfinite(out["c_grad"][1]).all()) and bool(torch.isfinite(out["a_grad"][1]).all())


def test_optional_outputs_may_be_null_and_no_rows_give_zero_gradients():
    from mdr_amd import _learner as L
    from mdr_amd import _native as nat
    from mdr_amd import maddpg as M
    n, f, h, b = 2, 5, 20, 16
    nets, data, index, noise_t, noise_a = _random_case(n, f, h, b)
    actors, critics, tgt_actors, tgt_critics = ([x[k] for x in nets] for k in range(4))
    lib = nat.load()
    adescs, cdescs, tadescs, tcdescs = (L.mlp_descs([L.fc_layers(m) for m in group]) for group in (actors, critics, tgt_actors, tgt_critics))
    a_floats, c_floats, _ = M._sizes(adescs[0], cdescs[0], n, b)
    ws = torch.empty(int(lib.mdr_maddpg_workspace_bytes_all(C.byref(adescs[0]), C.byref(cdescs[0]), n, b, 0)), dtype=torch.uint8, device=DEV)
    got = []
    for optional in (True, False):
        y, nq, na = torch.empty((n, b), device=DEV), torch.empty((n, b), device=DEV), torch.empty((n, b, n), dtype=torch.uint8, device=DEV)
        cg, cl, q = torch.empty((n, c_floats), device=DEV), torch.empty(n, device=DEV), torch.empty((n, b), device=DEV)
        ag, al, lg = torch.empty((n, a_floats), device=DEV), torch.empty(n, device=DEV), torch.empty((n, b, 2), device=DEV)
        with torch.cuda.device(DEV):
            st = L.stream(torch.device(DEV))
            M._target_all_launch(tadescs, tcdescs, data["next_state"], n * f, data["reward"], index, b, n, noise_t, y, nq if optional else None, na,
                                 st, 0.5, 0.99)
            M._critic_all_launch(cdescs, data["state"], n * f, data["action"], index, b, n, y, ws, cg, cl, q if optional else None, st)
            M._actor_all_launch(adescs, cdescs, data["state"], n * f, data["action"], index, b, n, noise_a, ws, ag, al, q if optional else None,
                                lg if optional else None, st, 0.5, M.PSE)
        got.append((y, na, cg, cl, ag, al))
    for x, z in zip(*got):
        assert torch.equal(x, z)
    cg, cl = torch.full((n, c_floats), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    with torch.cuda.device(DEV):      # no rows: the single call's zeros, for every agent
        M._critic_all_launch(cdescs, data["state"], n * f, data["action"], index, 0, n, y, ws, cg, cl, None, L.stream(torch.device(DEV)))
    assert not bool(cg.any()) and not bool(cl.any())


# ---- step_nets -------------------------------------------------------------------------------------------------------------------------
# three nets of unequal sizes: 42 floats (its bias a slice that starts at the odd float 35), 3.3 k, and 77 k - above the 70804 floats up
# to which FusedAdam.step is one launch, so the comparison covers both of its forms
NET_SHAPES = [[(7, 5), (7,)], [(50, 60), (50,), (4, 50), (4,)], [(300, 256), (256,)]]
GRAD_SCALE = [1e-3, 1e-2, 1e-2]      # total norms of about 0.006, 0.57 and 2.8: the clip at 0.5 leaves net 0 alone and scales nets 1 and 2


def _adam_nets(seed):
    from mdr_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    params, targets, flats, opts = [], [], [], []
    for shapes in NET_SHAPES:
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen, device=DEV)) for s in shapes]
        flat = torch.empty(sum(p.numel() for p in ps), device=DEV)
        off = 0
        for p in ps:
            p.grad = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        params.append(ps), flats.append(flat), targets.append([torch.randn(s, generator=gen, device=DEV) for s in shapes])
        opts.append(FusedAdam(ps, 3e-3))
    return params, targets, flats, opts, gen


@pytest.mark.parametrize("blend", [False, True], ids=["no_blend", "blend"])
@pytest.mark.parametrize("clip", [None, 0.5], ids=["no_clip", "clip"])
def test_step_nets_gives_the_bits_of_one_step_per_optimiser(clip, blend):
    from mdr_amd import optim
    one, two = _adam_nets(5), _adam_nets(5)
    assert (one[0][0][1].grad.data_ptr() // 4) % 2 == 1      # net 0's bias: a slice at an odd float offset
    for step in range(2):      # the second step starts from moments that are not zero
        for flat_a, flat_b, scale in zip(one[2], two[2], GRAD_SCALE):
            flat_a.normal_(generator=one[4]).mul_(scale)
            flat_b.copy_(flat_a)
        before = [f.clone() for f in one[2]]
        kw = dict(tau=0.25) if blend else {}
        norms = optim.step_nets(one[3], clip, targets=one[1] if blend else None, want_norm=True, **kw)
        want_norms = torch.stack([opt.step(max_grad_norm=clip, want_norm=True, **(dict(target=tgt, tau=0.25) if blend else {})).clone()
                                  for opt, tgt in zip(two[3], two[1])])
        assert torch.equal(norms, want_norms) and bool((norms > 0).all())
        if step == 0:
            assert float(norms[0]) < 0.5 < float(norms[1]) < float(norms[2])
        for k in range(len(NET_SHAPES)):
            for p, q in zip(one[0][k], two[0][k]):
                assert torch.equal(p, q), (k, step)
            assert torch.equal(one[3][k]._exp_avg, two[3][k]._exp_avg) and torch.equal(one[3][k]._exp_avg_sq, two[3][k]._exp_avg_sq)
            for t, u in zip(one[1][k], two[1][k]):
                assert torch.equal(t, u), (k, step)
            assert torch.equal(one[2][k], before[k])      # .grad is read, never written
            assert one[3][k].step_count() == two[3][k].step_count() == step + 1
    if not blend:      # the targets were not touched
        fresh = _adam_nets(5)[1]
        assert all(torch.equal(t, u) for ts, us in zip(one[1], fresh) for t, u in zip(ts, us))
    # either form continues the other: the state is the optimisers' own
    for flat_a, flat_b in zip(one[2], two[2]):
        flat_b.copy_(flat_a)
    for opt in one[3]:
        opt.step(max_grad_norm=clip)
    optim.step_nets(two[3], clip)
    assert all(torch.equal(p, q) for ps, qs in zip(one[0], two[0]) for p, q in zip(ps, qs))
    # optimisers at different step counts do not go together
    one[3][0].step()
    assert "step counts" in optim.nets_refusal(one[3])
    with pytest.raises(ValueError, match="step counts"):
        optim.step_nets(one[3], clip)


# ---- the learner -----------------------------------------------------------------------------------------------------------------------
def _learner(d, agent_steps, sampler="philox"):
    from mdr_amd.maddpg import MADDPGLearner
    from mdr_amd.optim import FusedAdam
    nets = _case_nets(d)
    learner = MADDPGLearner([x[0] for x in nets], [x[1] for x in nets], N, LR_A, LR_C, gamma=R.GAMMA, soft_tau=SOFT_TAU, gumbel_tau=TAU,
                            batch_size=B, buffer_capacity=64, backend="hip", optimizer=FusedAdam, shared=False, sampler=sampler,
                            agent_steps=agent_steps)
    for k in range(N):
        learner.tgt_actors[k].load_state_dict(nets[k][2].state_dict())
        learner.tgt_critics[k].load_state_dict(nets[k][3].state_dict())
    learner.buffer.push(_dev(d["state"]), _dev(d["action"]), _dev(d["reward"]), _dev(d["next_state"]))
    return learner


def _params(learner):
    return [p for nets in (learner.actors, learner.critics, learner.tgt_actors, learner.tgt_critics) for net in nets for p in net.parameters()]


def _moments(learner):
    return [m for opt in learner.actor_optimizers + learner.critic_optimizers for m in (opt._exp_avg, opt._exp_avg_sq)]


def _same(one, two):
    assert all(torch.equal(x, y) for x, y in zip(_params(one), _params(two)))
    assert all(torch.equal(x, y) for x, y in zip(_moments(one), _moments(two)))
    for a, b in zip(one.actor_optimizers + one.critic_optimizers, two.actor_optimizers + two.critic_optimizers):
        assert a.step_count() == b.step_count()


@pytest.fixture(scope="module")
def inputs():
    return R.inputs(40, N, F_LEN, H, H)


@pytest.mark.parametrize("sampler,updates", [("philox", 3), ("torch", 1)])
def test_the_batched_learner_keeps_the_sequential_learners_bits(inputs, sampler, updates):
    seq, bat = _learner(inputs, "sequential", sampler), _learner(inputs, "batched", sampler)
    assert seq.agent_steps == "sequential" and bat.agent_steps == "batched"
    calls = {"seq": [], "bat": []}

    def hook(name):
        def record(l, which, a):
            net = (l.critics if which == "critic" else l.actors)[a]
            calls[name].append((which, a, torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone(),
                                [p.detach().clone() for t in l.tgt_actors for p in t.parameters()]))
        return record

    seq.before_step, bat.before_step = hook("seq"), hook("bat")
    for u in range(updates):
        tgt_before = [p.detach().clone() for t in bat.tgt_actors for p in t.parameters()]
        calls["seq"].clear(), calls["bat"].clear()
        out_s, out_b = seq.update(seed=u), bat.update(seed=u)
        for x, y in zip(out_s, out_b):
            assert x.shape == y.shape == (N,) and torch.equal(x, y), u
        _same(seq, bat)
        assert seq.training_step == bat.training_step == u + 1
        # 2 N calls: the N critics in order after the critics' gradients, then the N actors
        assert [(c[0], c[1]) for c in calls["bat"]] == [("critic", a) for a in range(N)] + [("actor", a) for a in range(N)]
        by_key = {(c[0], c[1]): c for c in calls["seq"]}
        assert len(by_key) == 2 * N
        for which, a, grad, tgts in calls["bat"]:
            assert torch.equal(grad, by_key[(which, a)][2]), (which, a)      # .grad at the hook: the sequential learner's
            assert all(torch.equal(x, y) for x, y in zip(tgts, tgt_before)), (which, a)      # the target actors of before the update
        assert not all(torch.equal(x, y) for x, y in zip(tgt_before, (p for t in bat.tgt_actors for p in t.parameters())))      # ... blended after


def test_a_learner_may_change_its_form_between_updates_and_checkpoints_interchange(inputs):
    never, switched = _learner(inputs, "batched"), _learner(inputs, "batched")
    for x, y in zip(never.update(seed=0), switched.update(seed=0)):
        assert torch.equal(x, y)
    switched.agent_steps = "sequential"
    for x, y in zip(never.update(seed=1), switched.update(seed=1)):
        assert torch.equal(x, y)
    _same(never, switched)
    switched.agent_steps = "batched"
    for x, y in zip(never.update(seed=2), switched.update(seed=2)):
        assert torch.equal(x, y)
    _same(never, switched)
    fresh = _learner(inputs, "sequential")      # a checkpoint of the batched learner continues in a sequential one, and back
    fresh.load_network_dict(never.network_dict())
    fresh.training_step = never.training_step
    _same(never, fresh)
    for x, y in zip(never.update(seed=3), fresh.update(seed=3)):
        assert torch.equal(x, y)
    back = _learner(inputs, "batched")
    back.load_network_dict(fresh.network_dict())
    back.training_step = fresh.training_step
    for x, y in zip(never.update(seed=4), back.update(seed=4)):
        assert torch.equal(x, y)
    _same(never, back)


def test_optimisers_at_different_step_counts_take_their_own_steps(inputs):
    """A heterogeneous checkpoint: agent 0's optimisers one step ahead.  ``step_nets`` refuses them, the batched update steps every
    net on its own for that update - the sequential learner's bits still."""
    seq, bat = _learner(inputs, "sequential"), _learner(inputs, "batched")
    seq.update(seed=0), bat.update(seed=0)
    ahead = _learner(inputs, "sequential")
    ahead.update(seed=0), ahead.update(seed=1)
    d = seq.network_dict()
    d[0] = ahead.network_dict()[0]
    seq.load_network_dict(d), bat.load_network_dict(d)
    assert bat.critic_optimizers[0].step_count() == 2 and bat.critic_optimizers[1].step_count() == 1
    for x, y in zip(seq.update(seed=5), bat.update(seed=5)):
        assert torch.equal(x, y)
    _same(seq, bat)


def test_train_maddpg_takes_a_batched_learner():
    """tests/test_gpu_maddpg_agents_learner.py's loop test with the batched learner: the loop needs no change."""
    import mdr_amd
    from mdr_amd.maddpg import MADDPGLearner, train_maddpg
    from mdr_amd.optim import FusedAdam
    from tests.test_gpu_maddpg_agents_learner import _env, _twenty
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
    actors, critics = _twenty()
    learner = MADDPGLearner(actors, critics, 20, 1e-3, 3e-3, batch_size=8, buffer_capacity=64, backend="hip", shared=False, optimizer=FusedAdam,
                            agent_steps="batched")
    before = [a.fc[0].weight.detach().clone() for a in actors]
    a_losses, c_losses = train_maddpg(_env(cfg), learner, 4, update_every=2, random_steps=1, seed=2)
    assert a_losses.shape == (2, 20) and c_losses.shape == (2, 20)
    assert bool(torch.isfinite(a_losses).all()) and bool(torch.isfinite(c_losses).all())
    assert not torch.equal(a_losses[0], a_losses[1])      # the returned losses are the update's own tensors, not one reused buffer
    assert all(not torch.equal(a.fc[0].weight, w) for a, w in zip(actors, before))      # all 20 actors moved
