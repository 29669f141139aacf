"""Every ported learner's update against the REFERENCE's own ``update()``, on the CPU: the fixtures tests/golden/learner_*.npz were
recorded by running agents/ppo.py, agents/mappo.py, agents/dqn.py, agents/ddpg.py and agents/tarmac_ppo.py themselves (oracle/learner_golden.py), in float32 and as an fp64
twin.  Checked here: the fixtures exercise what they must; the ``*_grad_ref.evaluate`` restatements reproduce the reference's fp64
first-minibatch losses and gradients; each learner's ``backend="torch"`` on the CPU, fed the recorded draws, lands within
4 x d_ref32 of ref64 in every recorded quantity (tests/learner_golden.py); the project's return scan equals the reference's ``Gt``;
and, where the reference is present, a live re-run reproduces the committed fixtures."""
import numpy as np
import pytest
import torch

from oracle import learner_golden as rec
from oracle import ref_harness
from tests import learner_golden as lg

PPO_CASES = ("ppo_f51", "ppo_f21_zero", "tarmac_ppo")


@pytest.mark.parametrize("case", lg.CASES)
def test_fixture_exercises_what_it_must(case):
    lg.conditions(lg.fixture(case))


@pytest.mark.parametrize("case", lg.CASES)
def test_restatement_reproduces_the_references_fp64_first_minibatch(case):
    """rtol 1e-10 per element, with 1e-10 of the gradient's largest element as the absolute floor: an element that is a cancelling
    sum carries the rounding of its terms, not of its own size."""
    for net, r in lg.first_minibatch_reference(case).items():
        np.testing.assert_allclose(r["restated_loss"], r["loss"], rtol=1e-10, err_msg=net)
        np.testing.assert_allclose(r["restated_grad"], r["grad"], rtol=1e-10, atol=1e-10 * np.abs(r["grad"]).max(), err_msg=net)
        if "module_grad" in r:      # shared MADDPG: maddpg_grad_ref.evaluate itself
            np.testing.assert_allclose(r["module_loss"], r["loss"], rtol=1e-10, err_msg=net)
            np.testing.assert_allclose(r["module_grad"], r["grad"], rtol=1e-10, atol=1e-10 * np.abs(r["grad"]).max(), err_msg=net)
        assert np.abs(r["grad"]).max() > 1e-3      # nothing vacuous


@pytest.mark.parametrize("case", lg.CASES)
def test_torch_backend_on_the_cpu_lands_on_the_reference(case):
    res = lg.run_case(case, "torch", "cpu", **lg.stated_relation(case))
    lg.assert_within(lg.fixture(case), res, "torch cpu")
    for net, (loss, grad) in lg.first_minibatch_ratios(case, res).items():
        print("%s %s: first minibatch loss %.3f, gradient %.3f of the derived bound" % (case, net, loss, grad))
        assert loss <= 1.0 and grad <= 1.0, (net, loss, grad)
    if lg.fixture(case).kind == "maddpg":
        for net, ratio in lg.maddpg_actor_grad_ratios(case, res).items():
            print("%s %s: first gradient at %.2f of the reference's own float32 distance" % (case, net, ratio))
            assert ratio <= lg.FACTOR, (net, ratio)


def test_shared_maddpg_blends_once_where_the_reference_blends_twice():
    """The finding ``stated_relation`` describes, pinned from the other side: at the reference's own soft_tau the project's shared
    target nets are NOT the reference's (one blend against two), while its nets after the first update - which read the targets as
    the constructor left them - still are."""
    fx = lg.fixture("maddpg_shared")
    res = lg.run_case("maddpg_shared", "torch", "cpu")
    d = lg.d_ref32(fx)
    for net in ("tgt_actor0", "tgt_critic0"):
        first = max(np.abs(lg._kept(res.ckpt["first"][net])[k] - fx.checkpoint("ref64", "first", net)[k]).max() for k in fx.keys(net))
        assert first > 100 * d[net], net
        # one blend moves the target by tau (from - to), two by (2 tau - tau^2) (from - to): the gap is about tau of a step's change
    for net in ("actor0", "critic0"):
        first = max(np.abs(lg._kept(res.ckpt["first"][net])[k] - fx.checkpoint("ref64", "first", net)[k]).max() for k in fx.keys(net))
        assert first <= lg.FACTOR * d[net], net


def test_ddqn_target_net_stays_where_the_reference_leaves_it():
    """agents/dqn.py:119-146 never blends: both reference runs end on the initial target net, and so does soft_update=False."""
    fx = lg.fixture("ddqn_b1")
    for k in lg.FC_KEYS:
        kept = fx["init/policy/" + k].reshape(-1)[rec.ckpt_positions(fx["init/policy/" + k].shape)]
        assert np.array_equal(fx.checkpoint("ref64", "last", "target")[k], kept.astype(np.float64))
        assert np.array_equal(fx.checkpoint("ref32", "last", "target")[k], kept.astype(np.float64))
    assert lg.d_ref32(fx)["target"] == 0.0


def _returns(lay, gamma, bootstrap):
    from mdr_amd.rollout import discounted_returns
    boot = torch.from_numpy(bootstrap) if bootstrap is not None else None
    return discounted_returns(torch.from_numpy(lay["reward"]), torch.from_numpy(lay["done"]), gamma, boot).numpy().astype(np.float64)


@pytest.mark.parametrize("case", PPO_CASES)
def test_discounted_returns_equal_the_references_gt(case):
    """Two roundings per step of the float32 recurrence against the reference's Python-float loop: (T + 1) 2^-23 max|Gt|."""
    fx = lg.fixture(case)
    lay = lg.ppo_layout(fx)
    got = _returns(lay, fx.meta("gamma"), None if fx.meta("zero_eoepisode_return") else fx["ref32/bootstrap"])
    tol = (fx.meta("T") + 1) * 2.0 ** -23 * np.abs(lay["Gt32"]).max()
    assert np.abs(got - lay["Gt32"]).max() <= tol
    if not fx.meta("zero_eoepisode_return"):
        assert np.abs(fx["ref32/bootstrap"][-1]).min() > 1e-3


def test_mappo_returns_are_per_agent_not_the_references_storage_order():
    """agents/mappo.py:68-74 runs ONE recursion over the buffer as train_mappo.py:86 fills it - step-major, the agents interleaved - so
    within an episode a transition's return continues with the NEXT AGENT's of the same step.  The project scans each agent's own
    rewards (mdr_amd/mappo.py's docstring): it equals the reference's Gt of the same transitions stored agent by agent, and not the
    storage-order one."""
    fx = lg.fixture("mappo")
    lay = lg.ppo_layout(fx)
    T, N = fx.meta("T"), fx.meta("nb_agents")
    got = _returns(lay, fx.meta("gamma"), None)
    by_agent = fx.f64("ref32/Gt_by_agent").reshape(N, T).T
    tol = (T + 1) * 2.0 ** -23 * np.abs(by_agent).max()
    assert np.abs(got - by_agent).max() <= tol
    assert np.abs(got - lay["Gt32"]).max() > 1e-2      # the storage-order recursion is another function of the rewards
    # the stated relation: Gt[t, a] = r[t, a] + gamma * Gt of the next transition in storage order, reset where done
    r, g = lay["reward"].astype(np.float64).reshape(-1), lay["Gt32"].astype(np.float64).reshape(-1)
    done = lay["done"].reshape(-1)
    nxt = np.where(done, 0.0, np.append(g[1:], 0.0))
    assert np.abs(g - (r + fx.meta("gamma") * nxt)).max() <= 2.0 ** -22 * np.abs(g).max()


@pytest.mark.reference
@pytest.mark.parametrize("case", lg.CASES)
def test_live_rerun_reproduces_the_committed_fixture(case):
    if not ref_harness.available():
        pytest.skip("the reference is not installed here")
    live, fx = rec.generate(case), lg.fixture(case)
    assert sorted(live) == sorted(fx.a)
    for k in live:
        assert np.array_equal(np.asarray(live[k]), fx.a[k]), k
