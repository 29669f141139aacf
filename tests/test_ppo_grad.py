"""The yardstick of the PPO gradient kernels (tests/ppo_grad_ref.py) held to account on the CPU, and the host-only parts of the
feature: the ctypes mirror of mdr_mlp_t, the size helpers' refusals, PPOLearner.minibatches."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import ppo_grad_ref as pr
from tests.test_abi import _header, _struct_fields

HEADS = [2, 1]


def _case_id(c):
    return "B%d-F%d-H%d-%d" % c


@pytest.mark.parametrize("O", HEADS)
@pytest.mark.parametrize("net", pr.NETS, ids=lambda n: "F%d-H%d-%d" % n)
def test_draw_is_exact_and_exercises_every_rule(net, O):
    """On the 257-row draw every case of the network is a prefix of: z1, z2 bit-identical between fp64 and fp32 in two summation
    orders; about half the units active; pre-activations of exactly 0 occur; >= 99 % of the rows have p in [0.05, 0.95]; no ratio
    within 1e-3 of a clip bound and >= 10 % of the rows on each side of the gradient rule."""
    d = pr.inputs(pr.PARENT_ROWS, *net, O)
    f64, f32, f32p = pr.forward(d, np.float64), pr.forward(d, np.float32), pr.forward(d, np.float32, perm=True)
    for k in ("z1", "z2"):
        assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f32[k], f32p[k]), k
        assert 0.25 < (f64[k] > 0).mean() < 0.75, (k, (f64[k] > 0).mean())
    assert (f64["z1"] == 0).any()
    if O == 2:
        l = f64["l"]
        p0 = 1 / (1 + np.exp(l[:, 1] - l[:, 0]))
        assert ((p0 >= 0.05) & (p0 <= 0.95)).mean() >= 0.99
        ratio = pr.evaluate(d)["ratio"]
        assert (np.minimum(np.abs(ratio - 0.8), np.abs(ratio - 1.2)) >= 1e-3).all()
        adv = d["adv"].astype(np.float64)
        s1, s2 = ratio * adv, np.clip(ratio, 0.8, 1.2) * adv
        active = ((ratio >= 0.8) & (ratio <= 1.2)) | (s1 < s2)
        assert 0.1 <= active.mean() <= 0.9, active.mean()


@pytest.mark.parametrize("case", pr.SWEEP, ids=_case_id)
def test_every_case_is_exact_in_fp32(case):
    for O in HEADS:
        d = pr.inputs(*case, O)
        f64, f32, f32p = pr.forward(d, np.float64), pr.forward(d, np.float32), pr.forward(d, np.float32, perm=True)
        for k in ("z1", "z2"):
            assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f32[k], f32p[k]), (k, O)


@pytest.mark.parametrize("O", HEADS)
def test_closed_form_equals_autograd_of_the_reference_expression(O):
    """fp64 autograd of agents/ppo.py:148-169, 180 on the same inputs gives the closed-form gradient (to fp64 rounding)."""
    B, F, H1, H2 = 257, 51, 100, 100
    d = pr.inputs(B, F, H1, H2, O)
    ps = [torch.tensor(np.asarray(d[k], dtype=np.float64), requires_grad=True) for k in pr.PARAM_NAMES]
    x = torch.tensor(np.asarray(d["x"], dtype=np.float64))
    h = torch.relu(x @ ps[0].t() + ps[1])
    h = torch.relu(h @ ps[2].t() + ps[3])
    out = h @ ps[4].t() + ps[5]
    if O == 2:
        prob = torch.softmax(out, dim=1).gather(1, torch.from_numpy(d["action"].copy()).view(-1, 1))
        ratio = prob / torch.tensor(d["old"].astype(np.float64)).view(-1, 1)
        adv = torch.tensor(d["adv"].astype(np.float64)).view(-1, 1)
        loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - pr.CLIP, 1 + pr.CLIP) * adv).mean()
    else:
        loss = torch.nn.functional.mse_loss(torch.tensor(d["target"].astype(np.float64)).view(-1, 1), out)
    loss.backward()
    auto = np.concatenate([p.grad.numpy().reshape(-1) for p in ps])
    ref = pr.evaluate(d)
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-13
    assert np.abs(auto - ref["grad"]).max() < 1e-13


@pytest.mark.parametrize("case", pr.SWEEP, ids=_case_id)
def test_fp32_evaluations_stay_inside_the_bound(case):
    """An fp32 numpy evaluation of the formulas, in two summation orders, is inside the bound on every element of every output."""
    for O in HEADS:
        r = pr.reference(*case, O)
        for perm in (False, True):
            got = pr.evaluate(r["inputs"], np.float32, perm=perm)
            for k in r["bound"]:
                w = pr.worst(got[k], r["ref"][k], r["bound"][k])
                assert w <= 1.0, (O, perm, k, w)


@pytest.mark.parametrize("variant", pr.VARIANTS_ACTOR + pr.VARIANTS_CRITIC)
def test_wrong_variants_leave_the_bound(variant):
    """Each wrong variant is outside the bound on more than half of the elements of at least one parameter's gradient."""
    O = 1 if variant in pr.VARIANTS_CRITIC else 2
    case = (257, 51, 100, 100)
    r = pr.reference(*case, O)
    got = pr.evaluate(r["inputs"], np.float32, variant=variant)
    ratio = pr.ratio_to_bound(got["grad"], r["ref"]["grad"], r["bound"]["grad"])
    fractions = {n: float((ratio[s] > 1).mean()) for n, s in pr.param_slices(*case[1:], O).items()}
    assert max(fractions.values()) > 0.5, fractions


def test_ctypes_mirror_of_mdr_mlp_matches_header():
    assert _struct_fields(_header(), "mdr_mlp") == [f[0] for f in nat.MdrMlp._fields_]


def _net(F, H1, H2, O, size=None):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, F, H1, H2, O)


def test_size_helpers_refuse_shapes_outside_the_limits():
    """Host-only calls: no GPU needed."""
    lib = nat.load()
    assert lib.mdr_mlp_grad_floats(C.byref(_net(51, 100, 100, 2))) == 100 * 51 + 100 + 100 * 100 + 100 + 2 * 100 + 2
    assert lib.mdr_mlp_grad_floats(C.byref(_net(64, 128, 128, 1))) == 128 * 64 + 128 + 128 * 128 + 128 + 128 + 1
    for bad in ((65, 100, 100, 2), (51, 129, 100, 2), (51, 100, 129, 2), (51, 100, 100, 3), (0, 100, 100, 2), (51, 100, 100, 0)):
        assert lib.mdr_mlp_grad_floats(C.byref(_net(*bad))) == -1, bad
        assert lib.mdr_mlp_grad_workspace_bytes(C.byref(_net(*bad)), 256, 0) == -1, bad
    assert lib.mdr_mlp_grad_floats(C.byref(_net(51, 100, 100, 2, size=8))) == -1
    assert lib.mdr_mlp_grad_floats(None) == -1
    net = _net(51, 100, 100, 2)
    stride = (lib.mdr_mlp_grad_floats(C.byref(net)) + 1 + 3) // 4 * 4 * 4
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), 33, 2) == 2 * stride          # 3 tiles of 16 rows, 2 workgroups
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), 17, 8) == 2 * stride          # never more workgroups than tiles
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), 0, 0) == stride
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), 10 ** 7, 0) == 512 * stride   # the library's own grid on any device
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), -1, 0) == -1
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(net), 16, -1) == -1


def test_minibatches_cover_every_transition_once():
    from mdr_amd.ppo import PPOLearner
    from mdr_amd.rollout import ActorMLP, CriticMLP
    learner = PPOLearner(ActorMLP(8, layers=(16, 16)), CriticMLP(8, layers=(16, 16)), 1e-3, 1e-3, batch_size=256, backend="torch")
    n = 1000
    a = learner.minibatches(n, seed=3, epoch=0)
    assert [len(b) for b in a] == [256, 256, 256, 232]          # the short last batch is kept
    assert torch.equal(torch.sort(torch.cat(a)).values, torch.arange(n))
    again = learner.minibatches(n, seed=3, epoch=0)
    assert all(torch.equal(p, q) for p, q in zip(a, again))
    assert not torch.equal(torch.cat(a), torch.cat(learner.minibatches(n, seed=3, epoch=1)))
    assert not torch.equal(torch.cat(a), torch.cat(learner.minibatches(n, seed=4, epoch=0)))
