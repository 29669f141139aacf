"""The wide entry points (include/mdr_policy.h: mdr_*_wide, 65..128 input features) on the host: the size helpers, every refusal
that needs no device, the `wide=` keyword's defaults - and tests/ppo_grad_ref.py, the fp64 yardstick of the GPU tests, held to
account at the new widths: the draws are exact in fp32 and exercise every rule there as they do at 51 features, so the derived
bound tests/test_gpu_wide_grad.py asserts means at 121 features what it means at 51."""
import ctypes as C

import numpy as np
import pytest

from mdr_amd import _native as nat
from tests import dqn_grad_ref as dr
from tests import mappo_grad_ref as mr
from tests import ppo_grad_ref as pr

# (F, H1, H2).  The message columns' widths with the reference's hidden sizes: 121 (both flags), 81 (thermal), 91 (hvac); 65: the
# first width past the narrow limit (a fifth feature block); 128: the widest; 100 / 101: ld1 steps from 100 to 132; a narrow
# hidden pair at the widest input; no size a multiple of 16; 128-128 at its widest input, the tightest LDS fit
MAIN = (121, 100, 100)
NETS = [MAIN, (65, 100, 100), (81, 100, 100), (91, 100, 100), (128, 100, 100), (100, 100, 100), (101, 100, 100), (128, 64, 64),
        (97, 113, 97), (100, 128, 128)]
ROWS = [1, 15, 16, 17, 33, 65, 257]
SWEEP = [(B,) + MAIN for B in ROWS] + [(B,) + net for net in NETS[1:] for B in (65, 257)]
# the joint critic (B, F, N, H1, H2): J = F + N - 1 = 110, 110 and 128, all past the 100 inputs the un-aliased layout holds at 100-100
JOINT_SHAPES = [(51, 60, 100, 100), (91, 20, 100, 100), (121, 8, 100, 100)]
JOINT_SWEEP = [(B,) + s for s in JOINT_SHAPES for B in (65, 257)]
# bit-equality with the narrow entry points: the reference's shape and the narrow limits' corner
NARROW = [(51, 100, 100), (64, 128, 128)]
HEADS = [2, 1]

WIDE = {"mdr_mlp_grad_floats": "mdr_mlp_wide_grad_floats", "mdr_mlp_grad_workspace_bytes": "mdr_mlp_wide_grad_workspace_bytes",
        "mdr_ppo_actor_grad": "mdr_ppo_actor_grad_wide", "mdr_ppo_critic_grad": "mdr_ppo_critic_grad_wide",
        "mdr_dqn_target": "mdr_dqn_target_wide", "mdr_dqn_grad": "mdr_dqn_grad_wide",
        "mdr_mappo_critic_grad_floats": "mdr_mappo_critic_wide_grad_floats",
        "mdr_mappo_critic_workspace_bytes": "mdr_mappo_critic_wide_workspace_bytes", "mdr_mappo_critic_grad": "mdr_mappo_critic_grad_wide"}


def _case_id(c):
    return "B%d-F%d-H%d-%d" % c


def _net_id(n):
    return "F%d-H%d-%d" % n


# ---- the yardstick at the new widths

# The two nets at the ld1 step are this file's own addition; the others carry the figures the feature was specified with, which are
# whole per cent (one decimal for the share of unsaturated rows) and are compared at that precision: a share of 0.4556 is "46 %".
STEP_NETS = [(100, 100, 100), (101, 100, 100)]


def _percent(x):
    return int(np.floor(100.0 * x + 0.5))


@pytest.mark.parametrize("O", HEADS, ids=["actor", "critic"])
@pytest.mark.parametrize("net", NETS, ids=_net_id)
def test_draw_is_exact_and_exercises_every_rule_at_the_wide_shapes(net, O):
    """On the 257-row draw every case of the network is a prefix of: z1, z2 bit-identical between fp64 and fp32 in two summation
    orders; 46-56 % of the units active; pre-activations of exactly 0 occur in z1; at least 99.6 % of the rows have p in
    [0.05, 0.95]; no ratio within 1e-3 of a clip bound; 71-79 % of the rows on the active side of the gradient rule.
    STEP_NETS, which those figures were not taken for, meet what tests/test_ppo_grad.py asks of the narrow draws (a quarter to three
    quarters of the units active, at least a tenth of the rows on either side of the rule), and 95 % of their rows have p in
    [0.05, 0.95]: a saturated row has a gradient near 0, which the bound covers like any other; the condition only keeps the bulk
    of the rows where the softmax's rounding matters."""
    d = pr.inputs(pr.PARENT_ROWS, *net, O)
    own = net in STEP_NETS
    f64, f32, f32p = pr.forward(d, np.float64), pr.forward(d, np.float32), pr.forward(d, np.float32, perm=True)
    for k in ("z1", "z2"):
        assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f32[k], f32p[k]), k
        active = float((f64[k] > 0).mean())
        print("%s O%d %s active %.4f" % (net, O, k, active))
        assert (25 <= _percent(active) <= 75) if own else (46 <= _percent(active) <= 56), (k, active)
    assert (f64["z1"] == 0).any()
    if O == 2:
        l = f64["l"]
        p0 = 1 / (1 + np.exp(l[:, 1] - l[:, 0]))
        inside = float(((p0 >= 0.05) & (p0 <= 0.95)).mean())
        ratio = pr.evaluate(d)["ratio"]
        assert (np.minimum(np.abs(ratio - 0.8), np.abs(ratio - 1.2)) >= 1e-3).all()
        adv = d["adv"].astype(np.float64)
        s1, s2 = ratio * adv, np.clip(ratio, 0.8, 1.2) * adv
        on = float((((ratio >= 0.8) & (ratio <= 1.2)) | (s1 < s2)).mean())
        print("%s p inside %.4f, active side %.4f" % (net, inside, on))
        assert inside >= (0.95 if own else 0.996), inside
        assert (10 <= _percent(on) <= 90) if own else (71 <= _percent(on) <= 79), on


@pytest.mark.parametrize("case", SWEEP, ids=_case_id)
def test_every_wide_case_is_exact_and_fp32_stays_far_inside_the_bound(case):
    """Every case of the GPU sweep: z1, z2 exact in fp32 in two orders, and an fp32 numpy evaluation of the formulas, in two
    summation orders, reaches at most 0.035 of the bound on every element of every output."""
    for O in HEADS:
        r = pr.reference(*case, O)
        d = r["inputs"]
        f64, f32, f32p = pr.forward(d, np.float64), pr.forward(d, np.float32), pr.forward(d, np.float32, perm=True)
        for k in ("z1", "z2"):
            assert np.array_equal(f64[k], f32[k].astype(np.float64)) and np.array_equal(f32[k], f32p[k]), (k, O)
        for perm in (False, True):
            got = pr.evaluate(d, np.float32, perm=perm)
            for k in r["bound"]:
                w = pr.worst(got[k], r["ref"][k], r["bound"][k])
                assert w <= 0.035, (O, perm, k, w)


@pytest.mark.parametrize("double", [False, True], ids=["dqn", "ddqn"])
@pytest.mark.parametrize("net", [MAIN, (100, 128, 128)], ids=_net_id)
def test_dqn_yardstick_at_the_wide_shapes(net, double):
    """tests/dqn_grad_ref.py at the widest cases: no argmax is a matter of rounding (its draw's own margin rule), all three Huber
    branches occur, and an fp32 evaluation stays inside the bound with next_action exact."""
    r = dr.reference(257, *net, double)
    d = r["inputs"]
    assert dr._margin_ok(d, d["xn"]).all()
    delta = r["ref"]["q"] - r["ref"]["y"]
    assert (delta > 1).any() and (delta < -1).any() and (np.abs(delta) < 1).any()
    assert 0.25 <= r["ref"]["next_action"].mean() <= 0.75
    got = dr.evaluate(d, np.float32, double=double)
    assert np.array_equal(got["next_action"], r["ref"]["next_action"])
    for k in r["bound"]:
        assert dr.worst(got[k], r["ref"][k], r["bound"][k]) <= 1.0, k


@pytest.mark.parametrize("case", JOINT_SWEEP, ids=lambda c: "B%d-F%d-N%d-H%d-%d" % c)
def test_joint_yardstick_at_the_wide_shapes(case):
    r = mr.reference(*case)
    d = r["inputs"]
    F, N = case[1], case[2]
    assert d["x"].shape[1] == F + N - 1 > 100 and set(np.unique(d["x"][:, F:])) <= {0.0, 1.0}
    f64, f32 = pr.forward(d, np.float64), pr.forward(d, np.float32, perm=True)
    for k in ("z1", "z2"):
        assert np.array_equal(f64[k], f32[k].astype(np.float64)), k
    got = pr.evaluate(d, np.float32, perm=True)
    for k in r["bound"]:
        assert pr.worst(got[k], r["ref"][k], r["bound"][k]) <= 1.0, k


# ---- the C calls' host side: nothing below reaches a device

def _mlp(F=121, H1=100, H2=100, O=2, size=None, ptr=0x1000):
    return nat.MdrMlp(C.sizeof(nat.MdrMlp) if size is None else size, F, H1, H2, O, *([ptr] * 6))


def _floats(F, H1, H2, O):
    return H1 * F + H1 + H2 * H1 + H2 + O * H2 + O


def test_every_wide_entry_point_is_exported_with_its_sibling_s_signature():
    lib = nat.load()
    for narrow, wide in WIDE.items():
        assert wide in nat.EXPORTS
        a, b = getattr(lib, narrow), getattr(lib, wide)
        assert a.restype is b.restype and list(a.argtypes) == list(b.argtypes), wide


def test_wide_size_helpers():
    lib = nat.load()
    for net in NETS + NARROW + [(1, 1, 1), (128, 112, 112), (128, 96, 128)]:
        for O in HEADS:
            assert lib.mdr_mlp_wide_grad_floats(C.byref(_mlp(*net, O))) == _floats(*net, O), (net, O)
    # the limits and the LDS fit: hidden 100-100 fits at every width, 128-128 up to 100 inputs
    for F in range(1, 129):
        assert lib.mdr_mlp_wide_grad_floats(C.byref(_mlp(F, 100, 100, 1))) == _floats(F, 100, 100, 1), F
        assert (lib.mdr_mlp_wide_grad_floats(C.byref(_mlp(F, 128, 128, 2))) > 0) == (F <= 100), F
    for bad in ((129, 100, 100, 2), (121, 129, 100, 2), (121, 100, 129, 2), (101, 128, 128, 2), (128, 128, 128, 1), (121, 100, 100, 3),
                (0, 100, 100, 2), (121, 100, 100, 0)):
        assert lib.mdr_mlp_wide_grad_floats(C.byref(_mlp(*bad))) == -1, bad
        assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(_mlp(*bad)), 256, 0) == -1, bad
    assert lib.mdr_mlp_wide_grad_floats(C.byref(_mlp(size=8))) == -1 and lib.mdr_mlp_wide_grad_floats(None) == -1
    net = _mlp()
    stride = (_floats(121, 100, 100, 2) + 1 + 3) // 4 * 4 * 4
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), 33, 2) == 2 * stride
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), 17, 8) == 2 * stride
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), 0, 0) == stride
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), 10 ** 7, 0) == 512 * stride
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), -1, 0) == -1
    assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(net), 16, -1) == -1
    # where the narrow helpers answer, the wide ones give their answers; past 64 features the narrow ones still refuse
    for shape in NARROW:
        n = _mlp(*shape, 2)
        assert lib.mdr_mlp_wide_grad_floats(C.byref(n)) == lib.mdr_mlp_grad_floats(C.byref(n)) > 0
        assert lib.mdr_mlp_wide_grad_workspace_bytes(C.byref(n), 257, 3) == lib.mdr_mlp_grad_workspace_bytes(C.byref(n), 257, 3) > 0
    assert lib.mdr_mlp_grad_floats(C.byref(_mlp(65, 100, 100, 2))) == -1
    assert lib.mdr_mlp_grad_workspace_bytes(C.byref(_mlp(65, 100, 100, 2)), 256, 0) == -1


def test_wide_joint_size_helpers():
    lib = nat.load()
    for F, N, H1, H2 in JOINT_SHAPES:
        net = _mlp(F + N - 1, H1, H2, 1)
        assert lib.mdr_mappo_critic_wide_grad_floats(C.byref(net), N) == _floats(F + N - 1, H1, H2, 1)
        assert lib.mdr_mappo_critic_grad_floats(C.byref(net), N) == -1      # more than 100 joint inputs at 100-100: the wide layout alone
        stride = (_floats(F + N - 1, H1, H2, 1) + 1 + 3) // 4 * 4 * 4
        assert lib.mdr_mappo_critic_wide_workspace_bytes(C.byref(net), N, 33, 2) == 2 * stride
        assert lib.mdr_mappo_critic_wide_workspace_bytes(C.byref(net), N, -1, 0) == -1
        assert lib.mdr_mappo_critic_wide_workspace_bytes(C.byref(net), N, 16, -1) == -1
    for J in range(1, 129):
        assert lib.mdr_mappo_critic_wide_grad_floats(C.byref(_mlp(J, 100, 100, 1)), 1) > 0, J
        assert (lib.mdr_mappo_critic_wide_grad_floats(C.byref(_mlp(J, 128, 128, 1)), 1) > 0) == (J <= 100), J
    assert lib.mdr_mappo_critic_wide_grad_floats(C.byref(_mlp(140, 100, 100, 1)), 20) == -1      # F = 121 with 20 agents: J = 140
    for net, N in ((_mlp(129, 100, 100, 1), 9), (_mlp(128, 129, 100, 1), 8), (_mlp(128, 100, 129, 1), 8), (_mlp(101, 128, 128, 1), 8),
                   (_mlp(128, 100, 100, 2), 8), (_mlp(128, 100, 100, 1), 0), (_mlp(128, 100, 100, 1), 129), (_mlp(128, 100, 100, 1, size=8), 8)):
        assert lib.mdr_mappo_critic_wide_grad_floats(C.byref(net), N) == -1
        assert lib.mdr_mappo_critic_wide_workspace_bytes(C.byref(net), N, 256, 0) == -1
    # where both answer they agree
    net = _mlp(70, 100, 100, 1)
    assert lib.mdr_mappo_critic_wide_grad_floats(C.byref(net), 20) == lib.mdr_mappo_critic_grad_floats(C.byref(net), 20) > 0


UNSUPPORTED = (dict(F=129, ld=256), dict(H1=129), dict(H2=129), dict(F=101, H1=128, H2=128))


@pytest.mark.parametrize("O", HEADS, ids=["actor", "critic"])
def test_wide_ppo_calls_refuse_on_the_host(O):
    lib = nat.load()
    p = C.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch

    def call(net="default", state=p, ld=121, B=16, w0=p, w1=p, adv=p, clip=0.2, mw=0, ws=p, grad=p, loss=p):
        net = _mlp(O=O) if net == "default" else net
        ref = C.byref(net) if net is not None else None
        if O == 2:
            return lib.mdr_ppo_actor_grad_wide(ref, state, ld, None, B, w0, w1, adv, C.c_float(clip), mw, ws, grad, loss, None, None)
        return lib.mdr_ppo_critic_grad_wide(ref, state, ld, None, B, w0, mw, ws, grad, loss, None, None, None)

    invalid = [dict(net=None), dict(state=None), dict(w0=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ld=120), dict(B=-1),
               dict(mw=-1), dict(ws=C.c_void_p(0x1004)), dict(net=_mlp(O=O, size=8)), dict(net=_mlp(O=O, ptr=None))]
    if O == 2:
        invalid += [dict(w1=None), dict(adv=None), dict(clip=-0.1), dict(clip=1.0), dict(clip=float("nan"))]
    for kw in invalid:
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    for shape in UNSUPPORTED + (dict(O=3 - O), dict(O=3)):
        shape = dict(shape)
        ld = shape.pop("ld", 121)
        assert call(net=_mlp(**dict(dict(O=O), **shape)), ld=ld) == nat.MDR_ERR_UNSUPPORTED, shape


def test_wide_dqn_calls_refuse_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    net, pol = _mlp(), _mlp()

    def target(target=net, policy=None, ns=p, ld=121, B=16, reward=p, gamma=0.99, mw=0, y=p, na=p):
        return lib.mdr_dqn_target_wide(C.byref(target) if target is not None else None, C.byref(policy) if policy is not None else None, ns, ld,
                                       None, B, reward, C.c_float(gamma), mw, y, None, na, None)

    for kw in (dict(target=None), dict(ns=None), dict(reward=None), dict(y=None), dict(ld=120), dict(B=-1), dict(mw=-1), dict(gamma=float("nan")),
               dict(gamma=float("inf")), dict(target=_mlp(size=8)), dict(target=_mlp(ptr=None)), dict(policy=pol, na=None),
               dict(policy=_mlp(size=8)), dict(policy=_mlp(ptr=None))):
        assert target(**kw) == nat.MDR_ERR_INVALID, kw
    for shape in UNSUPPORTED + (dict(O=1), dict(O=3)):
        shape = dict(shape)
        ld = shape.pop("ld", 121)
        assert target(target=_mlp(**shape), ld=ld) == nat.MDR_ERR_UNSUPPORTED, shape
    for kw in (dict(policy=_mlp(F=120)), dict(policy=_mlp(H1=96)), dict(policy=_mlp(H2=96)), dict(policy=_mlp(O=1))):
        assert target(**kw) == nat.MDR_ERR_UNSUPPORTED, kw
    assert target(B=0) == nat.MDR_OK and target(B=0, policy=pol) == nat.MDR_OK      # zero rows: nothing to launch

    def grad(net=net, state=p, ld=121, B=16, action=p, y=p, clamp=1.0, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_dqn_grad_wide(C.byref(net) if net is not None else None, state, ld, None, B, action, y, C.c_float(clamp), mw, ws, grad, loss,
                                     None, None)

    for kw in (dict(net=None), dict(state=None), dict(action=None), dict(y=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ld=120),
               dict(B=-1), dict(mw=-1), dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(ws=C.c_void_p(0x1004)),
               dict(net=_mlp(size=8)), dict(net=_mlp(ptr=None))):
        assert grad(**kw) == nat.MDR_ERR_INVALID, kw
    for shape in UNSUPPORTED + (dict(O=1), dict(O=3)):
        shape = dict(shape)
        ld = shape.pop("ld", 121)
        assert grad(net=_mlp(**shape), ld=ld) == nat.MDR_ERR_UNSUPPORTED, shape


def test_wide_joint_call_refuses_on_the_host():
    lib = nat.load()
    p = C.c_void_p(0x1000)
    F, N = 121, 8
    net = _mlp(F + N - 1, 100, 100, 1)

    def call(net=net, state=p, ld=F, action=p, M=16 * N, N=N, B=16, target=p, mw=0, ws=p, grad=p, loss=p):
        return lib.mdr_mappo_critic_grad_wide(C.byref(net) if net is not None else None, state, ld, action, M, N, None, B, target, mw, ws, grad,
                                              loss, None, None, None)

    for kw in (dict(net=None), dict(state=None), dict(action=None), dict(target=None), dict(grad=None), dict(loss=None), dict(ws=None),
               dict(N=0), dict(N=-1), dict(N=F + N), dict(ld=F - 1), dict(M=16 * N + 1), dict(B=-1), dict(mw=-1), dict(ws=C.c_void_p(0x1004)),
               dict(net=_mlp(F + N - 1, 100, 100, 1, size=8)), dict(net=_mlp(F + N - 1, 100, 100, 1, ptr=None))):
        assert call(**kw) == nat.MDR_ERR_INVALID, kw
    # the shape alone is refused (M = 0 is a multiple of every nb_agents)
    for bad, agents in ((_mlp(129, 100, 100, 1), 9), (_mlp(140, 100, 100, 1), 20), (_mlp(128, 129, 100, 1), 8), (_mlp(128, 100, 129, 1), 8),
                        (_mlp(101, 128, 128, 1), 8), (_mlp(128, 100, 100, 2), 8)):
        assert call(net=bad, N=agents, M=0, ld=256) == nat.MDR_ERR_UNSUPPORTED, (bad.num_state, bad.hidden1, bad.hidden2, bad.num_out)


# ---- the Python keyword on CPU modules: the defaults are the narrow answers

def test_the_keyword_defaults_to_the_narrow_limits():
    import inspect

    from mdr_amd import dqn, mappo, ppo
    from mdr_amd.rollout import ActorMLP, CriticMLP
    for fn in (ppo.supported, ppo.actor_loss_backward, ppo.critic_loss_backward, dqn.supported, dqn.td_target, dqn.q_loss_backward,
               mappo.supported, mappo.joint_critic_loss_backward, ppo.PPOLearner.__init__, ppo.PPOLearner.from_config, dqn.DQNLearner.__init__,
               dqn.DQNLearner.from_config, mappo.MAPPOLearner.__init__, mappo.MAPPOLearner.from_config):
        assert inspect.signature(fn).parameters["wide"].default is False, fn
    assert ppo._WIDE == WIDE and ppo.MAX_STATE == 64 and ppo.MAX_STATE_WIDE == 128
    actor = ActorMLP(121)
    assert "at most 64 input features" in ppo._refusal(actor, 2)
    assert "GPU" in ppo._refusal(actor, 2, wide=True)                                   # the width passes; CPU parameters do not
    assert "at most 128 input features" in ppo._refusal(ActorMLP(129), 2, wide=True)
    learner = ppo.PPOLearner(actor, CriticMLP(121), 1e-3, 1e-3, backend="auto", wide=True)
    assert learner.wide and not learner.uses_kernels(256)                               # CPU parameters: auto stays with torch
    assert not ppo.PPOLearner(actor, CriticMLP(121), 1e-3, 1e-3).wide
    with pytest.raises(ValueError, match="backend='hip'"):
        ppo.PPOLearner(actor, CriticMLP(121), 1e-3, 1e-3, backend="hip", wide=True)
