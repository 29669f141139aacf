"""TarMACA2CLearner on the GPU: one update with backend="hip" against backend="torch" on copies.

The first minibatch starts from the same parameters on both backends, on the dyadic grids of tests/tarmac_a2c_ref.py: either
backend's gradient lies within that file's bound E_g of the fp64 gradient g, and the parameters after the clip and the first Adam
step are held to the fp64 step of tests/optim_ref.py on g within that file's rounding bound plus what E_g can move the step by - the
tolerance of tests/test_gpu_tarmac_critic_learner.py for the same comparison (its docstring derives it).  The eight tensors the update
does not reach are bit-unchanged.  Later minibatches start from parameters that already differ by roundings: there the losses must be
finite and the kernel path the same bits run after run."""
import copy

import numpy as np
import pytest
import torch

from tests import optim_ref as O
from tests import tarmac_a2c_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = R.SHAPES[2]      # N = 5, F = 22, C = 8, S = 36, K = 16
N, F_LEN, CC, S, K = SHAPE
T, BATCH, EPOCHS = 40, 16, 2
LR, MAX_NORM = 1e-3, 0.5
VC, EC = float(R.VALUE_COEF), float(R.ENTROPY_COEF)
EPS = 1e-8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _setup():
    from mdr_amd.tarmac_a2c import TarMACA2CPolicy
    d = R.inputs(T + 1, *SHAPE)
    torch.manual_seed(3)
    policy = TarMACA2CPolicy(F_LEN, state_size=S, comm_size=CC, key_size=K).to(DEV)
    with torch.no_grad():
        sd = policy.state_dict()
        for p, key in R.SD_KEYS.items():
            sd[key].copy_(_dev(d[p]))
    batch = {"state": _dev(d["obs"]).reshape(T + 1, N, F_LEN), "comm": _dev(d["comm"]).reshape(T + 1, N, CC), "action": _dev(d["action"][:T]),
             "return": _dev(d["ret"][:T]), "value": torch.zeros((T + 1, 1), device=DEV)}
    return d, policy, batch


def _learner(policy, backend, optimizer=torch.optim.Adam):
    from mdr_amd.tarmac_a2c import TarMACA2CLearner
    return TarMACA2CLearner(copy.deepcopy(policy), lr=LR, value_loss_coef=VC, entropy_coef=EC, max_grad_norm=MAX_NORM, nb_updates=EPOCHS,
                            batch_size=BATCH, backend=backend, optimizer=optimizer)


def _buffers(batch):
    return (batch["state"][:T].reshape(-1, N, F_LEN), batch["comm"][:T].reshape(-1, N, CC), batch["action"].reshape(-1, N),
            batch["return"].reshape(-1, N))


def _first_step_bound(d, idx):
    """-> (fp64 results, their bound, the fp64 reached parameters after the first step [nine arrays], their bound)."""
    case = {k: (v[:T] if k in R.PER_STEP else v) for k, v in d.items()}
    ref, bnd = R.evaluate(case, index=idx), R.bound(case, index=idx)
    sl = R.param_slices(F_LEN, CC, S)
    shapes = [d[k].shape for k in R.REACHED]
    g = [ref["grad"][sl[k]].reshape(s) for k, s in zip(R.REACHED, shapes)]
    E_g = [bnd["grad"][sl[k]].reshape(s) for k, s in zip(R.REACHED, shapes)]
    p = [np.asarray(d[k], dtype=np.float64) for k in R.REACHED]
    zeros = [np.zeros_like(x) for x in p]
    step, E_round = O.bound(p, g, zeros, zeros, 1, LR, max_norm=MAX_NORM)
    norm = float(np.sqrt(sum(float((x * x).sum()) for x in g)))
    E_norm = float(np.sqrt(sum(float((x * x).sum()) for x in E_g)))
    raw = MAX_NORM / (norm + 1e-6)
    if MAX_NORM / (norm + E_norm + 1e-6) >= 1.0:
        coef, E_coef = 1.0, 0.0
    else:
        coef = min(raw, 1.0)
        E_coef = coef * E_norm / (norm + 1e-6 - E_norm)
    total = []
    for x, Ex, Er in zip(g, E_g, E_round["p"]):
        xs, E_x = coef * x, coef * Ex + np.abs(x) * E_coef
        moved = LR * np.minimum(2.0, E_x * EPS / (np.maximum(np.abs(xs) - E_x, 0.0) + EPS) ** 2)
        total.append(Er + moved)
    return ref, bnd, step["p"], total


@pytest.mark.parametrize("fused", [False, True], ids=["adam", "fused_adam"])
def test_hip_backend_against_torch_backend(fused):
    from mdr_amd import tarmac_a2c as A
    from mdr_amd.optim import FusedAdam
    opt = FusedAdam if fused else torch.optim.Adam
    d, policy, batch = _setup()
    hip, ref = _learner(policy, "hip", opt), _learner(policy, "torch", opt)
    assert hip.uses_kernels(BATCH, N) and not ref.uses_kernels(BATCH, N)
    obs, comm, action, ret = _buffers(batch)
    index = hip.minibatches(T, 0, 0)[0]
    assert index.shape == (BATCH,)
    want, bnd, p64, E_p = _first_step_bound(d, index.cpu().numpy())
    # the gradient either path takes, on copies: within the bound of fp64
    probe = copy.deepcopy(policy)
    vl, al, en = A.loss_backward(probe, obs, comm, action, ret, VC, EC, index=index)
    flat = torch.cat([p.grad.reshape(-1) for p in A._reached(probe)]).cpu().numpy()
    w = R.worst(flat, want["grad"], bnd["grad"])
    print("first minibatch: kernel gradient worst |error| / bound = %.3f" % w)
    assert w <= 1.0 and R.worst(np.array([float(vl), float(al), float(en)]), want["losses"], bnd["losses"]) <= 1.0
    auto = copy.deepcopy(policy)
    tv, ta, te = A.dense_losses(auto, obs[index], comm[index], action[index], ret[index])
    (tv * VC + ta - te * EC).backward()
    flat_t = torch.cat([p.grad.reshape(-1) for p in A._reached(auto)]).cpu().numpy()
    wt = R.worst(flat_t, want["grad"], bnd["grad"])
    print("first minibatch: autograd gradient worst |error| / bound = %.3f" % wt)
    assert wt <= 1.0
    start = {k: p.detach().clone() for k, p in policy.named_parameters()}
    for name, lrn in (("hip", hip), ("torch", ref)):
        out = lrn.step_minibatch(obs, comm, action, ret, index)
        assert R.worst(np.array([float(t) for t in out]), want["losses"], bnd["losses"]) <= 1.0, name
        got = [p.detach().cpu().numpy() for p in A._reached(lrn.policy)]
        w = O.worst_ratio(got, p64, E_p)
        print("%s after the first minibatch: worst |p - fp64 step| / bound = %.3f" % (name, w))
        assert w <= 1.0, name
        assert all(not np.array_equal(a, np.asarray(d[k])) for a, k in zip(got, R.REACHED))      # every reached tensor stepped
        for k, p in lrn.policy.named_parameters():      # the unreached ones: bit-unchanged, no gradient
            if k.startswith("base.comm."):
                assert torch.equal(p, start[k]) and p.grad is None, (name, k)
    for ph, pt, E in zip(A._reached(hip.policy), A._reached(ref.policy), E_p):
        assert bool(((ph.detach() - pt.detach()).double().abs().cpu().numpy() <= 2 * E).all())
    flat_buf = hip.policy._mdr_flat_grad
    assert all(p.grad.untyped_storage().data_ptr() == flat_buf.untyped_storage().data_ptr() for p in A._reached(hip.policy))
    assert not hasattr(ref.policy, "_mdr_flat_grad")
    # the whole update, from the start, on fresh learners: finite losses on both, the kernel path the same bits twice
    runs = []
    for _ in range(2):
        lrn = _learner(policy, "hip", opt)
        v, a, e, count = lrn.update(batch, seed=0)
        assert count == EPOCHS * 3 and all(bool(torch.isfinite(t)) for t in (v, a, e))
        runs.append([p.detach().clone() for p in lrn.policy.parameters()] + [v, a, e])
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    full = _learner(policy, "torch", opt)
    v, a, e, count = full.update(batch, seed=0)
    assert count == EPOCHS * 3 and all(bool(torch.isfinite(t)) for t in (v, a, e))
    print("whole update: value loss hip %.6f, torch %.6f" % (float(runs[0][-3]), float(v)))


def test_auto_follows_the_measured_range_and_hip_refuses_what_the_kernels_do():
    from mdr_amd import tarmac_a2c as A
    _, policy, _ = _setup()
    auto = _learner(policy, "auto")
    for n in (1, 64, 128, 1024, 1025, 4096, 10 ** 6):
        assert auto.uses_kernels(n, N) == (A.AUTO_MIN_AGENT_ROWS <= n * N <= A.AUTO_MAX_AGENT_ROWS)
    assert auto.uses_kernels(128, 20) and auto.uses_kernels(256, 20) and not auto.uses_kernels(512, 20) and not auto.uses_kernels(128, 50)
    assert not auto.uses_kernels(1, 65)
    assert policy._act_kernels(1, 20) and policy._act_kernels(1024, 20) and not policy._act_kernels(4096, 20)
    two = A.TarMACA2CPolicy(F_LEN, num_hops=2).to(DEV)
    assert not A.supported(two) and not _learner(two, "auto").uses_kernels(16, N)
    with pytest.raises(ValueError, match="backend='hip'.*one hop"):
        _learner(two, "hip")
    with pytest.raises(ValueError, match="1 to 64"):
        A.loss_backward(policy, torch.zeros((2, 65, F_LEN), device=DEV), torch.zeros((2, 65, CC), device=DEV),
                        torch.zeros((2, 65), dtype=torch.int64, device=DEV), torch.zeros((2, 65), device=DEV))
    with pytest.raises(ValueError, match="index must"):
        A.loss_backward(policy, torch.zeros((2, N, F_LEN), device=DEV), torch.zeros((2, N, CC), device=DEV),
                        torch.zeros((2, N), dtype=torch.int64, device=DEV), torch.zeros((2, N), device=DEV),
                        index=torch.zeros(2, dtype=torch.int32, device=DEV))
