"""Every ported learner's HIP update against the REFERENCE's own ``update()``: the fixtures tests/golden/learner_*.npz (recorded by
running agents/ppo.py, agents/mappo.py, agents/dqn.py, agents/ddpg.py and agents/tarmac_ppo.py themselves, oracle/learner_golden.py) replayed through ``backend="hip"``,
eager (TarMAC-PPO also with ``critic_backend="hip"``), with torch's Adam and with FusedAdam, fed the recorded minibatch draws.

At the first minibatch the losses and the pre-clip gradients (DQN: the clamped ones) lie within the derived bound of the reference's
fp64 values; the parameters after the first and the last step - the target nets included - and every per-step loss and gradient norm
lie within 4 x d_ref32 of the fp64 twin, d_ref32 being the reference's own float32-to-fp64 distance (tests/learner_golden.py);
``training_step`` ends where the reference's does.  Where the port leaves the reference's text on purpose the run is made under the
relation ``tests/learner_golden.py: stated_relation`` states (shared MADDPG's blend count).  ``graph=True`` is not run here: it cannot take injected draws, and
tests/test_gpu_graph_update.py pins it to the eager philox bits.

Before mdr_maddpg_grad.hip summed the rows' loss terms as a tree, ``maddpg_shared`` with FusedAdam missed the yardstick in the series
``loss/critic1`` (ratio 5.90; now 2.88): profiles/learner_golden_README.md."""
import pytest
import torch

from tests import learner_golden as lg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _optimizer(name):
    if name == "adam":
        return torch.optim.Adam
    from mdr_amd.optim import FusedAdam
    return FusedAdam


@pytest.mark.parametrize("optimizer", ["adam", "fused"])
@pytest.mark.parametrize("case", lg.CASES)
def test_hip_update_lands_on_the_references(case, optimizer):
    res = lg.run_case(case, "hip", DEV, _optimizer(optimizer), **lg.stated_relation(case))
    first = lg.first_minibatch_ratios(case, res)
    for net, (loss, grad) in first.items():
        print("%s hip+%s %s: first minibatch loss %.3f, gradient %.3f of the derived bound" % (case, optimizer, net, loss, grad))
    ratios = lg.assert_within(lg.fixture(case), res, "hip+" + optimizer)
    print("%s hip+%s: worst ratio to d_ref32 %.2f, to the first-minibatch bound %.3f"
          % (case, optimizer, max(ratios.values()), max(max(v) for v in first.values())))
    for net, (loss, grad) in first.items():
        assert loss <= 1.0 and grad <= 1.0, (net, loss, grad)
    if lg.fixture(case).kind == "maddpg":      # the actors' first gradients read a critic that has stepped once: off the bound's grids
        for net, ratio in lg.maddpg_actor_grad_ratios(case, res).items():
            print("%s hip+%s %s: first gradient at %.2f of the reference's own float32 distance" % (case, optimizer, net, ratio))
            assert ratio <= lg.FACTOR, (net, ratio)
