"""MAPPO's centralised critic (mdr_mappo_critic_grad, include/mdr_policy.h) restated in numpy on the CPU: the joint input
torch.cat((state, others_actions)) of agents/mappo.py:87 built from the flat `action` buffer, then tests/ppo_grad_ref.py's critic
formulas, fp64 values and derived rounding bound on it.  tests/test_mappo_grad.py holds the restatement to account,
tests/test_gpu_mappo_grad.py holds the kernel to it.

The action columns are 0 / 1, on every dyadic grid of ppo_grad_ref: z1 and z2 stay exact in fp32 in any summation order and the
bound holds unchanged.  The buffer has M >= B transitions (M a multiple of N, collect_ppo_rollout's flat layout: the agent index runs
fastest); the minibatch is its first B rows unless a test passes an index."""
import functools

import numpy as np

from tests import ppo_grad_ref as pr

# (F, N, H1, H2): the reference's shape; 50 agents; a small one; the PPO heads' width limit; the first fifth k-block; the widest;
# no action columns; one
SHAPES = [(51, 20, 100, 100), (51, 50, 100, 100), (8, 3, 16, 16), (51, 14, 128, 128), (51, 15, 128, 128), (64, 65, 64, 64),
          (22, 1, 100, 100), (22, 2, 100, 100)]
SWEEP = [(B,) + s for s in SHAPES for B in (65, 257)] + [(B,) + SHAPES[0] for B in (1, 15, 16, 17, 33)]
WRONG_GATHERS = ("k_gt_a", "next_env", "own_slot")


def buffer_rows(B, N):
    """A buffer of whole env-steps with at least one transition behind the minibatch."""
    return N * (B // N + 1)


def others(action, N, wrong=None):
    """train_mappo.py:79-84 on the flat layout: row j = (env-step, agent a = j % N) gets the N actions of its env-step without its
    own, in agent order -> float64 [M, N - 1] of 0 / 1.  `wrong`: one of WRONG_GATHERS, deliberately wrong forms."""
    action = np.asarray(action).reshape(-1)
    M = action.shape[0]
    assert M % N == 0
    j = np.arange(M)
    a = (j % N)[:, None]
    k = np.arange(N - 1)[None, :]
    base = (j[:, None] - a)
    if wrong == "next_env":
        base = (base + N) % M
    src = base + k + ((k > a) if wrong == "k_gt_a" else (k >= a))
    if wrong == "own_slot":
        src = np.where(k == (a + 1) % max(N - 1, 1), j[:, None], src)
    return (action[src] != 0).astype(np.float64)


def case(B, F, N, H1, H2, M=None):
    """-> dict(inputs, ref, bound): `inputs` holds the network and the buffer (state [M, F], action [M], target [M]) and `x`, the
    joint input of the first B transitions; `ref` / `bound` are ppo_grad_ref's fp64 evaluation and bound of the critic on it."""
    M = buffer_rows(B, N) if M is None else M
    assert M >= B and M % N == 0
    J = F + N - 1
    d = dict(pr.inputs(M, J, H1, H2, 1))
    action = np.random.default_rng([7, F, N, H1, H2, M]).integers(0, 2, M).astype(np.int64)
    x = np.array(d["x"], dtype=np.float32)
    x[:, F:] = others(action, N)
    d.update(state=np.ascontiguousarray(x[:, :F]), action=action, buffer_target=d["target"], x=x[:B], target=d["target"][:B])
    return dict(inputs=d, ref=pr.evaluate(d, np.float64), bound=pr.bound(d))


def with_x(d, x):
    """The inputs with another joint image (a wrong gather's, a minibatch's)."""
    return dict(d, x=np.asarray(x, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def reference(B, F, N, H1, H2):
    """One case, computed once and shared read-only."""
    r = case(B, F, N, H1, H2)
    for group in (r["inputs"], r["ref"], r["bound"]):
        for t in group.values():
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
    return r
