"""mdr_amd.optim without a GPU: the fp64 restatement of tests/optim_ref.py against torch.optim.Adam + clip_grad_norm_ (and the blend of
agents/dqn.py:77-82 as DQNLearner.update_target_network writes it) in float64 on the CPU, FusedAdam's refusals, and the keys and shapes
of its state_dict."""
import numpy as np
import pytest
import torch

from mdr_amd import optim
from tests import optim_ref as ref

MAX_NORM, LR, TAU = 0.5, 1e-3, 0.01


def _grads(step):
    """Alternating: scale 3 (norm far above 0.5: clipped), scale 0.01 (norm below: not clipped)."""
    return ref.draw(ref.SIX, 100 + step, 3.0 if step % 2 == 0 else 0.01)


def test_fp64_restatement_is_torch_adam_with_clip_grad_norm_in_float64():
    params = [torch.nn.Parameter(torch.from_numpy(x).double()) for x in ref.draw(ref.SIX, 1)]
    target = [torch.from_numpy(x).double() for x in ref.draw(ref.SIX, 2)]
    opt = torch.optim.Adam(params, LR)
    p = [x.detach().numpy().copy() for x in params]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    tg = [x.numpy().copy() for x in target]
    worst, clipped = 0.0, []
    for t in range(1, 11):
        g = _grads(t)
        for q, x in zip(params, g):
            q.grad = torch.from_numpy(x).double()
        total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        with torch.no_grad():      # DQNLearner.update_target_network
            torch._foreach_mul_(target, 1.0 - TAU)
            torch._foreach_add_(target, [q.detach() for q in params], alpha=TAU)
        out = ref.step(p, g, m, v, t, LR, target=tg, tau=TAU, max_norm=MAX_NORM)
        p, m, v, tg = out["p"], out["m"], out["v"], out["target"]
        clipped.append(out["total_norm"] > MAX_NORM)
        assert abs(float(total) - out["total_norm"]) <= 1e-12 * out["total_norm"]
        for mine, theirs in zip(p + tg, [q.detach() for q in params] + target):
            worst = max(worst, float(np.abs(mine - theirs.numpy()).max()))
        for q, mm, vv in zip(params, m, v):
            assert np.abs(opt.state[q]["exp_avg"].numpy() - mm).max() <= 1e-12
            assert np.abs(opt.state[q]["exp_avg_sq"].numpy() - vv).max() <= 1e-12
    print("ten steps: largest |restatement - torch float64| over parameters and targets = %.2e" % worst)
    assert clipped == [t % 2 == 0 for t in range(1, 11)]      # both branches of the clip ran
    assert worst <= 1e-12


def test_a_dead_segment_is_skipped_and_the_clamp_comes_first():
    shapes = ref.SIX
    p, m, v, tg = (ref.draw(shapes, s) for s in (1, 2, 3, 4))
    v = [np.abs(x) for x in v]
    g = ref.draw(shapes, 5, 3.0)
    g[2] = None
    out = ref.step(p, g, m, v, 4, LR, target=tg, tau=TAU, max_norm=MAX_NORM, clamp=1.0)
    for key, before in (("p", p), ("m", m), ("v", v), ("target", tg)):
        assert np.array_equal(out[key][2], before[2].astype(np.float64))
        assert not np.array_equal(out[key][0], before[0].astype(np.float64))
    live = np.concatenate([np.clip(x, -1, 1).reshape(-1) for x in g if x is not None]).astype(np.float64)
    assert abs(out["total_norm"] - np.sqrt((live * live).sum())) <= 1e-12
    _, bnd = ref.bound(p, g, m, v, 4, LR, target=tg, tau=TAU, max_norm=MAX_NORM, clamp=1.0)
    assert all(not b[2].any() for b in (bnd["p"], bnd["m"], bnd["v"], bnd["target"]))
    assert all((b[0] > 0).all() for b in (bnd["p"], bnd["m"], bnd["v"], bnd["target"])) and bnd["total_norm"] > 0


def test_the_bound_holds_a_float32_numpy_evaluation_and_not_a_wrong_one():
    """The same step evaluated in float32 by numpy (pairwise sums, its own order) sits inside the bound; the step with the clip applied
    after the moments' update instead of before sits far outside."""
    shapes = ref.CASES["ragged"] + ref.SIX
    p, m, tg = (ref.draw(shapes, s) for s in (1, 2, 4))
    v = [np.abs(x) * np.float32(0.1) for x in ref.draw(shapes, 3)]
    g = ref.draw(shapes, 5, 3.0)
    want, bnd = ref.bound(p, g, m, v, 10, LR, target=tg, tau=TAU, max_norm=MAX_NORM)
    f = np.float32
    ss = f(0)
    for x in g:
        ss = f(ss + (x * x).sum(dtype=f))
    norm = np.sqrt(ss)
    coef = min(f(MAX_NORM) / f(norm + f(1e-6)), f(1))
    a, c2 = f(LR / (1 - 0.9 ** 10)), f(np.sqrt(1 - 0.999 ** 10))
    worst = ref.worst_ratio(norm, want["total_norm"], bnd["total_norm"])
    for i, x in enumerate(g):
        x = coef * x
        mn = f(0.9) * m[i] + f(1 - 0.9) * x
        vn = f(0.999) * v[i] + f(1 - 0.999) * (x * x)
        pn = p[i] - a * (mn / (np.sqrt(vn) / c2 + f(1e-8)))
        tn = f(1 - TAU) * tg[i] + f(TAU) * pn
        assert all(y.dtype == f for y in (mn, vn, pn, tn))
        worst = max(worst, *(ref.worst_ratio([y], [want[k][i]], [bnd[k][i]]) for k, y in (("p", pn), ("m", mn), ("v", vn), ("target", tn))))
        wrong = f(0.9) * m[i] + f(1 - 0.9) * g[i]
        assert ref.worst_ratio([wrong], [want["m"][i]], [bnd["m"][i]]) > 1e3
    print("float32 numpy evaluation: worst |error| / bound = %.3f" % worst)
    assert worst <= 1.0


def test_refusals_name_their_reason():
    one = torch.nn.Parameter(torch.zeros(3, 2))
    with pytest.raises(ValueError, match="on the GPU"):
        optim.FusedAdam([one], LR)
    with pytest.raises(ValueError, match="float32"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], LR)
    with pytest.raises(ValueError, match="at most 32"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(1)) for _ in range(33)], LR)
    with pytest.raises(ValueError, match="contiguous"):
        optim.FusedAdam([torch.zeros(4, 3).t().requires_grad_()], LR)
    with pytest.raises(ValueError, match="one param group"):
        optim.FusedAdam([{"params": [one]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], LR)
    assert not optim.supported([one]) and not optim.supported([])


def test_state_dict_keys_and_shapes_are_torch_adams(monkeypatch):
    """On the CPU the constructor's device check is the only thing in the way: with it lifted (and no library call: the state is host
    bookkeeping) FusedAdam's state_dict after a first gradient has torch.optim.Adam's keys, shapes, dtypes and param_groups."""
    monkeypatch.setattr(optim, "_refusal", lambda params: None)

    class _Lib:
        def mdr_adam_workspace_bytes(self, n):
            return 16

    monkeypatch.setattr(optim.nat, "load", lambda: _Lib())
    mine = [torch.nn.Parameter(torch.from_numpy(x)) for x in ref.draw(ref.SIX, 1)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    fused, adam = optim.FusedAdam(mine, LR), torch.optim.Adam(theirs, LR)
    for p, q in zip(mine, theirs):
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    adam.step()
    for i in range(len(mine)):
        fused._adopt(i)
    a, b = fused.state_dict(), adam.state_dict()
    assert a.keys() == b.keys() and len(a["param_groups"]) == 1
    assert a["param_groups"][0].keys() == b["param_groups"][0].keys()
    assert {k: v for k, v in a["param_groups"][0].items()} == {k: v for k, v in b["param_groups"][0].items()}
    assert a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys()
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, (i, k)
    # the moments are views of the two flat buffers, in parameter order
    off = 0
    for i, p in enumerate(mine):
        assert fused.state[p]["exp_avg"].data_ptr() == fused._exp_avg.data_ptr() + 4 * off
        assert fused.state[p]["exp_avg_sq"].data_ptr() == fused._exp_avg_sq.data_ptr() + 4 * off
        off += p.numel()
    # and torch's state loads: the moments land in the flat buffers
    fused.load_state_dict(adam.state_dict())
    for p, q in zip(mine, theirs):
        assert torch.equal(fused.state[p]["exp_avg"], adam.state[q]["exp_avg"]) and float(fused.state[p]["step"]) == 1.0
        assert fused.state[p]["exp_avg"].data_ptr() >= fused._exp_avg.data_ptr()
    adam2 = torch.optim.Adam(theirs, LR)
    adam2.load_state_dict(fused.state_dict())
    adam2.step()      # torch's Adam continues from FusedAdam's state_dict
    assert float(adam2.state[theirs[0]]["step"]) == 2.0
