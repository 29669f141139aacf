"""TarMAC A2C on the CPU: the numpy restatement of tests/tarmac_a2c_ref.py against the recorded reference cases
(tests/golden/tarmac_a2c_cases.npz), ``TarMACA2CPolicy.forward_dense`` under autograd against the same cases, the restatement's
rounding bound (holds for fp32 in permuted summation orders, is broken by every deliberately wrong variant), the admission of every
case of the GPU sweep, and the host-side pieces: config mapping, ValueErrors, the ctypes mirror of mdr_tarmac_a2c_net_t."""
import os
import re

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from mdr_amd import tarmac_a2c as A
from tests import tarmac_a2c_ref as R

CASES = R.load_cases()
SWEEP = [(B,) + s for s in R.SHAPES for B in R.STEPS]


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)) / max(float(np.max(np.abs(want))), 1e-300))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_in_fp64_equals_the_reference(name):
    c = CASES[name]
    got = R.evaluate(c["inputs"], np.float64, vc=c["vc"], ec=c["ec"])
    B, N = c["B"], c["N"]
    for key, mine in (("value", got["value"]), ("logits", got["logits"].reshape(B, N, 2)), ("x", got["x"].reshape(B, N, c["S"])),
                      ("comm_out", got["comm_out"]), ("p_attn", got["attn"]), ("losses", got["losses"])):
        assert _rel(mine, c[key]) <= 1e-12, (name, key, _rel(mine, c[key]))
    s = R.param_slices(c["F"], c["C"], c["S"])
    flat = R.golden_flat_grad(c)
    for p in R.REACHED:
        assert _rel(got["grad"][s[p]], flat[s[p]]) <= 1e-12, (name, p)
    assert sorted(c["no_grad"]) == sorted(k for k in c["sd"] if k.startswith("base.comm."))      # eight tensors, none of them reached


@pytest.mark.parametrize("name", sorted(CASES))
def test_policy_loads_the_reference_state_dict_and_autograd_reproduces_it(name):
    c = CASES[name]
    policy = R.make_policy(c)
    d = c["inputs"]
    obs, comm, ret, action = (torch.from_numpy(np.array(d[k])) for k in ("obs", "comm", "ret", "action"))
    value, logits, x, comm_out, attn = policy.forward_dense(obs, comm)
    for key, mine in (("value", value), ("logits", logits), ("x", x), ("comm_out", comm_out), ("p_attn", attn)):
        assert _rel(mine.detach().numpy(), c[key]) <= 2e-5, (name, key)
    vl, al, en = A.dense_losses(policy, obs, comm, action, ret)
    assert _rel(torch.stack([vl, al, en]).detach().numpy(), c["losses"]) <= 2e-5
    (vl * c["vc"] + al - en * c["ec"]).backward()
    missing = [k for k, p in policy.named_parameters() if p.grad is None]
    assert sorted(missing) == sorted(c["no_grad"]) and len(missing) == 8
    for k, p in policy.named_parameters():
        if p.grad is not None:
            assert _rel(p.grad.numpy(), c["grad"][k]) <= 1e-4, (name, k)
    # the same in fp64: the module is the reference's formula
    dbl = R.make_policy(c).double()
    vl, al, en = A.dense_losses(dbl, obs.double(), comm.double(), action, ret.double())
    (vl * c["vc"] + al - en * c["ec"]).backward()
    assert _rel(torch.stack([vl, al, en]).detach().numpy(), c["losses"]) <= 1e-12
    for k, p in dbl.named_parameters():
        if p.grad is not None:
            assert _rel(p.grad.numpy(), c["grad"][k]) <= 1e-11, (name, k)


def test_every_case_of_the_sweep_is_admitted_and_z1_is_exact():
    left_out = [case for case in SWEEP if not R.admitted(R.reference(*case)["ref"], R.reference(*case)["bound"])]
    assert left_out == []
    for case in SWEEP:
        d = R.reference(*case)["inputs"]
        assert R.z1_is_exact(d), case
    zeros = sum(int((R.reference(*case)["ref"]["z1"] == 0).sum()) for case in SWEEP)
    masks = np.concatenate([R.reference(*case)["ref"]["m"].reshape(-1) > 0 for case in SWEEP])
    assert zeros > 100 and 0.2 < masks.mean() < 0.8      # z1 = 0 occurs; both sides of the critic's LeakyReLU


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B%d-N%d-F%d-C%d-S%d-K%d" % c)
def test_fp32_in_permuted_orders_stays_inside_the_bound(case):
    r = R.reference(*case)
    for perm in (False, True):
        got = R.evaluate(r["inputs"], np.float32, perm=perm)
        for k in R.FLOAT_KEYS:
            assert R.worst(got[k], r["ref"][k], r["bound"][k]) <= 1.0, (case, perm, k)


def _variant_cases(variant):
    cases = [(3,) + R.SHAPES[2], (3,) + R.SHAPES[4], (3,) + R.SHAPES[0]]
    return cases


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_breaks_the_bound(variant):
    broken = []
    for case in _variant_cases(variant):
        d = R.inputs(8, *case[1:])
        idx = np.array([5, 2, 7]) if variant == "ret_not_gathered" else None
        ref, bnd = R.evaluate(d, index=idx), R.bound(d, index=idx)
        got = R.evaluate(d, np.float32, variant=variant, index=idx)
        right = R.evaluate(d, np.float32, index=idx)
        assert R.worst_of(right, ref, bnd) <= 1.0
        broken += [k for k in R.FLOAT_KEYS if R.worst(got[k], ref[k], bnd[k]) > 1.0]
    print(variant, sorted(set(broken)))
    assert broken, variant


def test_index_is_the_gathered_copy():
    d = R.inputs(8, *R.SHAPES[2])
    idx = np.array([5, 2, 5, 7])
    a = R.evaluate(d, index=idx)
    b = R.evaluate(dict(d, obs=d["obs"][idx], comm=d["comm"][idx], ret=d["ret"][idx], action=d["action"][idx]))
    for k in R.FLOAT_KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_from_config_maps_the_reference_block():
    prop = {"recurrent_policy": True, "state_size": 128, "communication_size": 32, "tarmac_communication_mode": "from_states_rec_att",
            "comm_num_hops": 1, "value_loss_coef": 0.5, "entropy_coef": 0.01, "tarmac_lr": 7e-4, "tarmac_eps": 1e-5, "tarmac_gamma": 0.99,
            "tarmac_alpha": 0.99, "tarmac_max_grad_norm": 0.5, "distributed": False, "nb_tarmac_updates": 10, "tarmac_batch_size": 128}
    policy = A.TarMACA2CPolicy.from_config(prop, 22)      # recurrent_policy of the config is overridden, as in a2c_acktr.py:35
    assert (policy.nb_obs, policy.state_size, policy.comm_size, policy.key_size, policy.num_hops) == (22, 128, 32, 16, 1)
    learner = A.TarMACA2CLearner.from_config(prop, policy)
    assert (learner.value_loss_coef, learner.entropy_coef, learner.max_grad_norm, learner.nb_updates, learner.batch_size) == (0.5, 0.01, 0.5, 10, 128)
    group = learner.optimizer.param_groups[0]
    assert isinstance(learner.optimizer, torch.optim.Adam) and group["lr"] == 7e-4 and group["eps"] == 1e-8      # only lr is passed
    assert len(group["params"]) == 17 and learner.backend == "auto"
    assert not learner.uses_kernels(128, 20)      # a CPU policy: torch


def test_value_errors():
    with pytest.raises(ValueError, match=r"a2c_acktr\.py:35"):
        A.TarMACA2CPolicy(22, recurrent_policy=True)
    with pytest.raises(ValueError, match="num_hops"):
        A.TarMACA2CPolicy(22, num_hops=0)
    policy = A.TarMACA2CPolicy(22)
    assert not A.supported(policy) and "GPU" in A._refusal(policy)      # on the CPU
    assert "one hop" in A._refusal(A.TarMACA2CPolicy(22, num_hops=2))
    assert "multiple of 4" in A._refusal(A.TarMACA2CPolicy(22, state_size=30))
    assert "features" in A._refusal(A.TarMACA2CPolicy(129))
    assert "key_size" in A._refusal(A.TarMACA2CPolicy(22, key_size=20))
    assert "kernels cover a TarMACA2CPolicy" in A._refusal(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="backend must be"):
        A.TarMACA2CLearner(policy, backend="cuda")
    with pytest.raises(ValueError, match="backend='hip'"):
        A.TarMACA2CLearner(policy, backend="hip")
    with pytest.raises(ValueError, match="obs must be"):
        policy.forward_dense(torch.zeros(4, 22), torch.zeros(4, 32))
    with pytest.raises(ValueError, match="on the GPU"):
        policy.act(torch.zeros(1, 4, 22), torch.zeros(1, 4, 32), 0, 0)
    with pytest.raises(ValueError):
        A.loss_backward(policy, torch.zeros(1, 4, 22), torch.zeros(1, 4, 32), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4))


def test_two_hops_run_through_msg2nextstate_on_the_dense_path():
    policy = A.TarMACA2CPolicy(6, state_size=8, comm_size=4, key_size=4, num_hops=2)
    obs, comm = torch.randn(2, 3, 6), torch.randn(2, 3, 4)
    value, logits, x, comm_out, attn = policy.forward_dense(obs, comm)
    assert comm_out.shape == (2, 3, 4) and attn.shape == (2, 3, 3) and value.shape == (2,)
    comm_out.sum().backward()
    assert policy.base.comm.msg2nextstate[0].weight.grad is not None


def test_torch_learner_takes_one_adam_step_over_the_reached_parameters():
    torch.manual_seed(0)
    policy = A.TarMACA2CPolicy(6, state_size=8, comm_size=4, key_size=4)
    before = {k: p.detach().clone() for k, p in policy.named_parameters()}
    T, E, N = 3, 2, 3
    batch = dict(state=torch.randn(T + 1, E * N, 6), comm=torch.randn(T + 1, E * N, 4), action=torch.randint(0, 2, (T, E * N)),
                 value=torch.zeros(T + 1, E), **{"return": torch.randn(T, E * N)})
    learner = A.TarMACA2CLearner(policy, nb_updates=2, batch_size=4, backend="torch")
    vl, al, en, count = learner.update(batch, seed=1)
    assert count == 4 and all(t.dim() == 0 and bool(torch.isfinite(t)) for t in (vl, al, en))
    for k, p in policy.named_parameters():
        changed = not torch.equal(p, before[k])
        assert changed != k.startswith("base.comm."), k


def test_ctypes_mirror_matches_the_header():
    from tests.test_abi import _header, _struct_fields
    assert _struct_fields(_header(), "mdr_tarmac_a2c_net") == [f[0] for f in nat.MdrTarmacA2CNet._fields_]
    for name in ("mdr_tarmac_a2c_grad_floats", "mdr_tarmac_a2c_workspace_bytes", "mdr_tarmac_a2c_forward", "mdr_tarmac_a2c_comm", "mdr_tarmac_a2c_grad"):
        assert name in nat.EXPORTS and re.search(r"\b%s\s*\(" % name, _header())
    lib = nat.load()
    import ctypes as C
    net = nat.MdrTarmacA2CNet(C.sizeof(nat.MdrTarmacA2CNet), 22, 32, 128, 16)
    assert lib.mdr_tarmac_a2c_grad_floats(C.byref(net)) == 128 * 54 + 128 + 2 * (128 * 128 + 128) + 128 + 1 + 256
    assert lib.mdr_tarmac_a2c_workspace_bytes(C.byref(net), 128, 20, 0) == 4 * (4 * 2560 * 128 + 4 * 2560 + 4 * 128 * 128 + 5 * 128)
    assert lib.mdr_tarmac_a2c_workspace_bytes(C.byref(net), 128, 65, 0) == -1
    # host-side refusals: nothing is launched for a NULL pointer or a shape outside the limits
    assert lib.mdr_tarmac_a2c_forward(C.byref(net), None, 22, None, 32, None, 1, 20, 0, None, None, None, None, None) == nat.MDR_ERR_INVALID
    net.state_size = 132
    assert lib.mdr_tarmac_a2c_grad_floats(C.byref(net)) == -1
