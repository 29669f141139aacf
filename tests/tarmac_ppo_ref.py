"""The yardstick of the TarMAC-PPO actor gradient (mdr_tarmac_ppo_actor_grad, include/mdr_policy.h): inputs built on the recorded
reference actors of tests/golden/tarmac_actor_cases.npz, and the reference's own formula (agents/tarmac_ppo.py:168-186 on the dense
TarMAC_Actor.forward) evaluated under torch autograd on the CPU in float64 - and once more in float32, which is the error scale the
kernels are held to (the contract of tests/test_gpu_tarmac_grad.py::test_differentiable_forward_end_to_end).

Inputs.  ``action`` is drawn; ``old_prob = p64[action] * r`` (rounded to float32) with r from R_GRID, so every ratio is 1 / r up to
rounding: 1.4286, 1.1111, 1, 0.9091, 0.7692 - at least 0.03 from the clip bounds 0.8 and 1.2, five orders of magnitude more than
float32 moves a ratio; ``advantage`` comes from a signed grid, so all four (sign, clipped) branches occur in every case.

The ReLU condition.  relu'(z) is a step: a pre-activation that float32 and float64 put on different sides of 0 moves a whole row of a
weight gradient by O(1) without either evaluation being wrong.  ``build`` therefore asserts that no ReLU pre-activation of the
float64 forward (obs2hidden.0 and the head's first layer) lies within 2^-18 of 0 relative to its layer's largest |z| - float32
evaluates these sums of at most 96 terms to a few 2^-24 of that scale.  The recorded observations satisfy it (smallest margin
3.2e-5, f22_n20_c10); synthetic observations are N(0, 1/4) draws from the first seed that does, found on the CPU and written into
SYNTHETIC below (``first_seed``).
"""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import tarmac_ref as tr

CLIP = 0.2
R_GRID = (0.7, 0.9, 1.0, 1.1, 1.3)
ADV_GRID = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
RELU_MARGIN = 2.0 ** -18
FACTOR, FLOOR = 8.0, 2.0 ** -20      # test_differentiable_forward_end_to_end's E2E_FACTOR, E2E_FLOOR

ONE_HOP = ("f22_n20_c10", "f22_n20_nocomm", "f22_n20_none", "f22_n6_c0", "f51_n2_c10", "f51_n5_c3")
# name -> (recorded weights, N, B env-steps, max_workgroups, seed of the observations: the first that meets the ReLU condition)
SYNTHETIC = {
    "tiles_n13_b9": ("f22_n20_c10", 13, 9, 2, 0),        # 117 agents: an env straddles every tile edge, 4 tile pairs on 2 workgroups, a partial tile
    "band_n300_b2": ("f22_n20_c10", 300, 2, 2, 0),       # the band crosses tile edges inside an env
    "grid_plus_one": ("f51_n5_c3", 5, 1640, 0, 0),       # 8200 agents: one env-step beyond 256 workgroups x 32 agents; H = 8
}
DEFECT_PROB, DEFECT_SEED = 0.3, 0x1234567890ABCDEF
# two (seed, step) keys whose masks keep the ReLU condition on f22_n20_c10's recorded observations (found on the CPU: with step
# (3 << 32) + 0xFFFFFFFE one pre-activation of the head comes within 1.2e-6 of 0); the second has a high word
DEFECT_STEPS = (5, (3 << 32) + 0xFFFFFFFD)


def _relu_margin(actor64, obs64, dead):
    """The smallest |z| / max |z| over the ReLU pre-activations of each of the two ReLU layers."""
    seen = []
    head = actor64.comm_hidden2action if actor64.with_comm else actor64.hidden2action
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append(out.detach())) for m in (actor64.obs2hidden[0], head[0])]
    with torch.no_grad():
        actor64.dense_logits(obs64, dead)
    for h in hooks:
        h.remove()
    return min(float(z.abs().min() / z.abs().max()) for z in seen)


def _logits(actor, obs, dead):
    """``dense_logits``, except in mode "none": there the reference's masked softmax is 0 / 0 -> NaN -> 0, comm = 0 for every input,
    and autograd differentiates the 0 / 0 into NaN for every tensor upstream of it.  The gradient of the function the forward
    computes - comm identically 0 - is taken instead: the head sees [x, 0], the three projections get exact zeros (what
    mdr_tarmac_comm_backward documents for MDR_TARMAC_NONE)."""
    if actor.with_comm and actor.comm_mode == "none":
        x = actor.obs2hidden(obs)
        return actor.comm_hidden2action(torch.cat([x, x.new_zeros(x.shape[:2] + (actor.num_value,))], dim=2))
    return actor.dense_logits(obs, dead)


def _evaluate(actor, obs, action, old_prob, adv, dead):
    """agents/tarmac_ppo.py:168-186 in the dtype of ``actor`` -> (loss, ratio [B, N], {parameter name: gradient}) as float64 numpy."""
    actor.zero_grad()
    dt = next(actor.parameters()).dtype
    prob = F.softmax(_logits(actor, obs.to(dt), dead), dim=-1).gather(2, action.unsqueeze(2)).squeeze(2)
    ratio = prob / old_prob.to(dt)
    a = adv.to(dt)
    loss = -torch.min(ratio * a, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * a).mean()
    loss.backward()
    grads = {n: p.grad.detach().double().numpy().copy() for n, p in actor.named_parameters() if p.grad is not None}
    if actor.with_comm and actor.comm_mode == "none":
        grads.update({n: np.zeros(tuple(p.shape)) for n, p in actor.comm.named_parameters(prefix="comm") if "msg_state2state" not in n})
    return float(loss.detach()), ratio.detach().double().numpy(), grads


def rel_l2(got, ref):
    """name -> ||got - ref|| / ||ref|| per parameter tensor; where ||ref|| is below 1e-6 of the case's largest gradient norm (a
    gradient that vanishes exactly: hidden2key's last bias always, the query and key projections when a receiver hears itself alone)
    the error is taken relative to that largest norm - test_gpu_tarmac_grad.py's _rel_l2."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    top = max(np.linalg.norm(r) for r in ref.values())
    assert top > 0
    return {n: float(np.linalg.norm(got[n] - ref[n]) / (np.linalg.norm(ref[n]) if np.linalg.norm(ref[n]) > 1e-6 * top else top)) for n in ref}


def build(weights, obs, seed=0, defect=None):
    """One case on the float32 observations ``obs`` [B, N, F] with the recorded actor ``weights``.  ``defect``: (prob, seed, step) of
    the dead senders (tarmac_ref.dead_mask, the batch row as the env).  -> dict(case, actor (CPU, float32, dense), state, action,
    old_prob, adv, dead, loss, ratio, grad {name: float64}, yard {name: relative L2 error of the float32 CPU evaluation}, margin)."""
    case = tr.load_cases()[weights]
    obs = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32))
    B, N, _ = obs.shape
    prob = defect[0] if defect else 0.0
    actor = tr.make_actor(case, attention="dense", defect_prob=prob)
    dead = None
    if defect and case["with_comm"] and case["mode"] == tr.NEIGHBOURS:
        dead = torch.from_numpy(tr.dead_mask(B, N, prob, defect[1], defect[2]))
    a64 = copy.deepcopy(actor).double()
    margin = _relu_margin(a64, obs.double(), dead)
    assert margin > RELU_MARGIN, "ReLU condition: a pre-activation %.2e of its layer's largest (need > %.2e)" % (margin, RELU_MARGIN)
    rng = np.random.default_rng([seed, 0x7A, B, N])
    action = torch.from_numpy(rng.integers(0, 2, (B, N)).astype(np.int64))
    with torch.no_grad():
        p64 = F.softmax(_logits(a64, obs.double(), dead), dim=-1).gather(2, action.unsqueeze(2)).squeeze(2)
    r = torch.from_numpy(rng.choice(R_GRID, (B, N)))
    old_prob = (p64 * r).float()
    adv = torch.from_numpy(rng.choice(ADV_GRID, (B, N)).astype(np.float32))
    loss, ratio, grad = _evaluate(a64, obs, action, old_prob, adv, dead)
    assert np.abs(ratio - 1 / r.numpy()).max() < 1e-6
    assert min(np.abs(ratio - (1 - CLIP)).min(), np.abs(ratio - (1 + CLIP)).min()) > 0.03
    s1, s2 = ratio * adv.numpy(), np.clip(ratio, 1 - CLIP, 1 + CLIP) * adv.numpy()
    clipped, positive = s2 < s1, adv.numpy() > 0
    if B * N >= 40:
        for sign in (False, True):
            for cl in (False, True):
                assert ((positive == sign) & (clipped == cl)).any(), "branch (positive %s, clipped %s) does not occur" % (sign, cl)
    _, _, g32 = _evaluate(actor, obs, action, old_prob, adv, dead)
    actor.zero_grad(set_to_none=True)
    return dict(case=case, actor=actor, state=obs, action=action, old_prob=old_prob, adv=adv, dead=dead, loss=loss, ratio=ratio, grad=grad,
                yard=rel_l2(g32, grad), margin=margin)


@functools.lru_cache(maxsize=None)
def recorded(name, defect_step=None):
    """The recorded case ``name`` at B = 4 env-steps on its recorded observations; computed once, shared, not to be modified."""
    case = tr.load_cases()[name]
    return build(name, case["obs"], defect=(DEFECT_PROB, DEFECT_SEED, defect_step) if defect_step is not None else None)


def synthetic_obs(weights, N, B, seed):
    F_ = tr.load_cases()[weights]["F"]
    return (0.5 * np.random.default_rng([seed, 0x0B, N, B]).standard_normal((B, N, F_))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    weights, N, B, max_wg, seed = SYNTHETIC[name]
    d = build(weights, synthetic_obs(weights, N, B, seed), seed=seed)
    d["max_workgroups"] = max_wg
    return d


def first_seed(weights, N, B, limit=64):
    """The first seed whose synthetic observations meet the ReLU condition (how the seeds of SYNTHETIC were found)."""
    case = tr.load_cases()[weights]
    a64 = tr.make_actor(case, attention="dense").double()
    for seed in range(limit):
        if _relu_margin(a64, torch.from_numpy(synthetic_obs(weights, N, B, seed)).double(), None) > RELU_MARGIN:
            return seed
    raise AssertionError("no seed below %d meets the ReLU condition" % limit)


def holds(got, ref):
    """The contract per tensor: ``got`` {name: gradient} against the case ``ref`` -> (worst ratio error / max(yardstick, floor / factor),
    its tensor, {name: error}); the assertion is error <= max(FACTOR * yardstick, FLOOR) for every tensor."""
    err = rel_l2(got, ref["grad"])
    score = {n: err[n] / max(ref["yard"][n], FLOOR / FACTOR) for n in err}
    worst = max(score, key=score.get)
    return score[worst], worst, err
