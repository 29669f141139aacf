"""MADDPG's update step on the GPU (include/mdr_policy.h: mdr_maddpg_target, mdr_maddpg_critic_grad, mdr_maddpg_actor_grad).

The reference's default trainer (cli.py:38, main.py:38-47; agents/ddpg.py, train_ddpg.py).  ``MADDPG.update`` (ddpg.py:305-339) runs
once for every agent a: a fresh minibatch of env-steps, every agent's next action from the target actor through a hard
gumbel-softmax, ``y = reward_a + gamma * tgt_critic(cat(next_states, next_actions))``, the critic's mse step, then the actor's step on
``-critic(cat(states, actions with a's replaced by its own straight-through sample)).mean() + 1e-3 * logits.pow(2).mean()``; each step
clips the gradient norm to 0.5 and takes Adam; ``update_target`` then blends both target nets.  The centralised critic reads J =
N (F + 2) inputs - 1060 at the reference's 20 agents - through 256 hidden units: weights that do not fit LDS, so these kernels stream
them from L2 (csrc/mdr_maddpg_grad.hip) and leave the other learners' kernels as they are.  ``maddpg_target``,
``joint_q_loss_backward`` and ``actor_loss_backward`` are two launches each; ``JointReplayBuffer`` holds env-steps as preallocated
device tensors the kernels read in place through the sampled indices; ``MADDPGLearner`` is the update, ``train_maddpg`` the loop.
The gumbel noise is an input of every call, drawn by the learner - under a seeded generator or, with ``sampler="philox"``, by one launch
of mdr_maddpg_draws together with the minibatches: every backend sees the same noise.  ``graph=True`` replays a whole update from one
captured graph (graph_update.MADDPGUpdateGraph).  ``agent_steps="batched"`` (per-agent networks only) takes the N agents through every
stage of an update together - mdr_maddpg_target_all, mdr_maddpg_critic_grad_all, mdr_maddpg_actor_grad_all and ``optim.step_nets`` -
with the bits of the agents one after the other.  Nothing on the call path synchronises with the host.

Places that leave the reference's text on purpose:

* train_ddpg.py:86-91 and :111-115 store agent 0's observation for every agent.  Here every agent stores its own.
* The sharing block of ``MADDPG.__init__`` sits outside the loop (ddpg.py:217-223): under ``DDPG_shared: True`` only the last agent
  shares with agent 0.  Here there is one actor, one critic and one target of each for all agents - what the flag means and what every
  other learner of this project does - ``MADDPGLearner(shared=True)``, the default.  ``shared=False`` is the reference's other
  setting, which every checkpoint of ``saveDDPGDict`` holds: one actor, critic and target of each PER AGENT.  Acting then goes
  through ``FusedMLPActors`` and the target's picks through ``mdr_maddpg_target_agents`` (agent k's next action from agent k's own
  target actor); the critic's and the actor's step read agent a's nets alone and use the same kernels as the shared mode.
* ``MADDPG.update_target`` calls ``agent.update_target()`` once per entry of ``self.agents`` (ddpg.py:300-303): nets that several
  entries alias are blended once PER ALIASING ENTRY and update - with two agents, where the sharing block above does share
  everything, twice: to <- (1 - tau)^2 to + (1 - (1 - tau)^2) from.  ``MADDPGLearner(shared=True)`` blends its one pair of targets
  once per update with ``soft_tau``; ``soft_tau = 2 tau - tau^2`` reproduces the reference's two-agent run (tests/learner_golden.py:
  ``stated_relation``).  Unshared nets are blended once each, as in the reference.
* There is no terminal mask, as in ``mdr_dqn_target``: the reference's env never ends.
* The actor step does not write the critic's ``.grad``.  The reference pollutes it and zeroes it before its next use: unobservable.
* The clip norm is the literal 0.5 of ddpg.py:157 and :163; ``DDPG_prop["max_grad_norm"]`` is read by nobody in the reference.
"""
from __future__ import annotations

import copy
import ctypes as C
from functools import partial
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _learner as L
from . import _native as nat
from . import graph_update
from .optim import FusedAdam, nets_refusal, step_nets

MAX_STATE, MAX_HIDDEN, MAX_JOINT = 64, 256, 1280      # the kernels' limits (include/mdr_policy.h: mdr_maddpg_*)
# backend="auto": the kernels for minibatches of this many rows (profiles/maddpg_update_README.md: they measured 2.3-2.9x faster than
# autograd per update at 64 and 256 rows and 0.6-0.7x at 4096; nothing between was measured, so auto stays with the largest size they won)
AUTO_MIN_ROWS = 1
AUTO_MAX_ROWS = 256
# ... and for unshared per-agent networks (MADDPGLearner(shared=False)): torch, until profiles/maddpg_agents_README.md holds a table in
# which the kernels won at 64 and 256 rows by three times the run-to-run spread
AUTO_UNSHARED = False
PSE = 1e-3      # ddpg.py:339


class DDPGNetworkMLP(nn.Module):
    """agents/network.py:80-100 (``DDPG_Network``): Linear - ReLU - Linear - ReLU - Linear in an ``nn.Sequential`` named ``net``, Xavier-
    uniform weights with the ReLU gain, biases 0.01; state_dict keys ``net.0|2|4.weight|bias``, so the nets of ``saveDDPGDict`` load
    with ``load_state_dict``."""

    def __init__(self, in_dim: int, out_dim: int, hidden_dim: int = 256):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, out_dim))
        gain = nn.init.calculate_gain("relu")
        for m in self.net:
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight, gain=gain)
                m.bias.data.fill_(0.01)

    @property
    def fc(self):
        """The three Linear layers, as the gradient helpers of _learner.py index them."""
        return [self.net[0], self.net[2], self.net[4]]

    def forward(self, x):
        return self.net(x)


def _refusal(actor, critic, nb_agents: int) -> Optional[str]:
    """Why the kernels do not take this pair (None: they do)."""
    fa, fc = L.fc_layers(actor), L.fc_layers(critic)
    if fa is None or fc is None:
        return "the kernels cover Linear-ReLU-Linear-ReLU-Linear (DDPGNetworkMLP, or an `fc` list of three biased Linear layers)"
    for f in (fa, fc):
        if f[1].in_features != f[0].out_features or f[2].in_features != f[1].out_features:
            return "the three layers do not chain"
        if f[0].out_features > MAX_HIDDEN or f[1].out_features > MAX_HIDDEN:
            return "hidden layers of %d and %d units: the kernels cover at most %d" % (f[0].out_features, f[1].out_features, MAX_HIDDEN)
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in L.mlp_params(f)):
            return "parameters must be contiguous float32 tensors on the GPU"
    F_len = fa[0].in_features
    if int(nb_agents) < 1 or fc[0].in_features != int(nb_agents) * (F_len + 2):
        return "the critic must read nb_agents * (num_state + 2) = %d inputs, not %d" % (int(nb_agents) * (F_len + 2), fc[0].in_features)
    if F_len > MAX_STATE or fc[0].in_features > MAX_JOINT:
        return "num_state = %d, joint input = %d: the kernels cover at most %d and %d" % (F_len, fc[0].in_features, MAX_STATE, MAX_JOINT)
    if fa[2].out_features != 2 or fc[2].out_features != 1:
        return "the kernels cover an actor of 2 actions and a critic of 1 value"
    return None


def supported(actor, critic, nb_agents: int) -> bool:
    """Do the kernels take this actor and critic?  Two hidden layers of at most 256 units each (any size), an actor on F <= 64 features
    with 2 actions, a critic on nb_agents * (F + 2) <= 1280 inputs with 1 value, float32 on the GPU."""
    return _refusal(actor, critic, nb_agents) is None


def _check_steps(actor, state, index, nb_agents, what):
    """``state`` [M, N, F] (or [M, N F]) float32 with unit inner strides and an env-step stride >= N F -> (dev, M, ld, B)."""
    fa = L.fc_layers(actor)
    dev, F_len, N = fa[0].weight.device, fa[0].in_features, int(nb_agents)
    if state.dim() == 3:
        ok = state.shape[1:] == (N, F_len) and (F_len == 1 or state.stride(2) == 1) and (N == 1 or state.stride(1) == F_len)
    else:
        ok = state.dim() == 2 and state.shape[1] == N * F_len and (N * F_len == 1 or state.stride(1) == 1)
    if not ok or state.dtype != torch.float32 or state.device != dev:
        raise ValueError("%s: state must be a float32 [M, %d, %d] tensor on %s with contiguous env-steps" % (what, N, F_len, dev))
    M = int(state.shape[0])
    if M > 1 and state.stride(0) < N * F_len:
        raise ValueError("%s: the env-step stride must be >= nb_agents * F" % what)
    L.check_index(index, dev, what)
    ld = int(state.stride(0)) if M > 1 else N * F_len
    return dev, M, ld, (int(index.shape[0]) if index is not None else M)


def _is_seq(nets) -> bool:
    return isinstance(nets, (list, tuple))


def _agents_refusal(actors, critic, nb_agents: int) -> Optional[str]:
    """Why the per-agent kernels do not take these N actors with this critic (None: they do)."""
    actors = list(actors)
    if len(actors) != int(nb_agents):
        return "%d actors for %d agents" % (len(actors), int(nb_agents))
    if len(actors) > nat.MDR_MAX_AGENT_NETS:
        return "%d per-agent networks: the kernels cover at most %d" % (len(actors), nat.MDR_MAX_AGENT_NETS)
    for k, actor in enumerate(actors):
        why = _refusal(actor, critic, nb_agents)
        if why:
            return "agent %d: %s" % (k, why)
    shape = [lin.weight.shape for lin in L.fc_layers(actors[0])]
    for k, actor in enumerate(actors):
        if [lin.weight.shape for lin in L.fc_layers(actor)] != shape:
            return "agent %d's actor has another shape than agent 0's" % k
    return None


# -- the launches, on caller-owned buffers: what the functional wrappers below call and what a captured update records -----------------
def _sizes(adesc, cdesc, N: int, B: int, max_workgroups: int = 0) -> Tuple[int, int, int]:
    """(floats of the actor's flat gradient, of the critic's, bytes of workspace of either gradient call over B rows)."""
    lib = nat.load()
    return (int(lib.mdr_maddpg_grad_floats(C.byref(adesc))), int(lib.mdr_maddpg_grad_floats(C.byref(cdesc))),
            int(lib.mdr_maddpg_workspace_bytes(C.byref(adesc), C.byref(cdesc), N, B, max_workgroups)))


def _target_launch(tgt_actors, cdesc, next_state, ld, reward, index, B, N, agent, noise, y, next_q, next_action, st, tau, gamma,
                   max_workgroups: int = 0) -> None:
    """mdr_maddpg_target (``tgt_actors``: one ``mdr_mlp_t``) or mdr_maddpg_target_agents (a host array of N) on stream ``st``."""
    lib = nat.load()
    if isinstance(tgt_actors, nat.MdrMlp):
        name = "mdr_maddpg_target"
        rc = lib.mdr_maddpg_target(C.byref(tgt_actors), C.byref(cdesc), L.ptr(next_state), ld, L.ptr(reward), L.ptr(index), B, N, int(agent),
                                   L.ptr(noise), C.c_float(tau), C.c_float(gamma), max_workgroups, L.ptr(y), L.ptr(next_q), L.ptr(next_action), st)
    else:
        name = "mdr_maddpg_target_agents"
        rc = lib.mdr_maddpg_target_agents(tgt_actors, N, C.byref(cdesc), L.ptr(next_state), ld, L.ptr(reward), L.ptr(index), B, N, int(agent),
                                          L.ptr(noise), C.c_float(tau), C.c_float(gamma), max_workgroups, L.ptr(y), L.ptr(next_q),
                                          L.ptr(next_action), st)
    nat.check(lib, None, rc, name)


def _critic_launch(cdesc, state, ld, action, index, B, N, y, workspace, flat, loss, q, st, max_workgroups: int = 0) -> None:
    lib = nat.load()
    rc = lib.mdr_maddpg_critic_grad(C.byref(cdesc), L.ptr(state), ld, L.ptr(action), L.ptr(index), B, N, L.ptr(y), max_workgroups, L.ptr(workspace),
                                    L.ptr(flat), L.ptr(loss), L.ptr(q), st)
    nat.check(lib, None, rc, "mdr_maddpg_critic_grad")


def _actor_launch(adesc, cdesc, state, ld, action, index, B, N, agent, noise, workspace, flat, loss, q, logits, st, tau, pse,
                  max_workgroups: int = 0) -> None:
    lib = nat.load()
    rc = lib.mdr_maddpg_actor_grad(C.byref(adesc), C.byref(cdesc), L.ptr(state), ld, L.ptr(action), L.ptr(index), B, N, int(agent), L.ptr(noise),
                                   C.c_float(tau), C.c_float(pse), max_workgroups, L.ptr(workspace), L.ptr(flat), L.ptr(loss), L.ptr(q),
                                   L.ptr(logits), st)
    nat.check(lib, None, rc, "mdr_maddpg_actor_grad")


def _target_all_launch(tgt_adescs, tgt_cdescs, next_state, ld, reward, index, B, N, noise, y, next_q, next_action, st, tau, gamma,
                       max_workgroups: int = 0) -> None:
    """mdr_maddpg_target_all: every agent's y on its own minibatch; the descriptors are host arrays of N (``_learner.mlp_descs``)."""
    lib = nat.load()
    rc = lib.mdr_maddpg_target_all(tgt_adescs, tgt_cdescs, L.ptr(next_state), ld, L.ptr(reward), L.ptr(index), B, N, L.ptr(noise), C.c_float(tau),
                                   C.c_float(gamma), max_workgroups, L.ptr(y), L.ptr(next_q), L.ptr(next_action), st)
    nat.check(lib, None, rc, "mdr_maddpg_target_all")


def _critic_all_launch(cdescs, state, ld, action, index, B, N, y, workspace, flat, loss, q, st, max_workgroups: int = 0) -> None:
    lib = nat.load()
    rc = lib.mdr_maddpg_critic_grad_all(cdescs, L.ptr(state), ld, L.ptr(action), L.ptr(index), B, N, L.ptr(y), max_workgroups, L.ptr(workspace),
                                        L.ptr(flat), L.ptr(loss), L.ptr(q), st)
    nat.check(lib, None, rc, "mdr_maddpg_critic_grad_all")


def _actor_all_launch(adescs, cdescs, state, ld, action, index, B, N, noise, workspace, flat, loss, q, logits, st, tau, pse,
                      max_workgroups: int = 0) -> None:
    lib = nat.load()
    rc = lib.mdr_maddpg_actor_grad_all(adescs, cdescs, L.ptr(state), ld, L.ptr(action), L.ptr(index), B, N, L.ptr(noise), C.c_float(tau),
                                       C.c_float(pse), max_workgroups, L.ptr(workspace), L.ptr(flat), L.ptr(loss), L.ptr(q), L.ptr(logits), st)
    nat.check(lib, None, rc, "mdr_maddpg_actor_grad_all")


def maddpg_target(tgt_actor, tgt_critic, next_state: torch.Tensor, reward: torch.Tensor, agent: int, noise: torch.Tensor,
                  tau: float = 1.0, gamma: float = 0.99, index: Optional[torch.Tensor] = None, max_workgroups: int = 0
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``target_value`` of ddpg.py:317-322 for agent ``agent`` -> (y, next_q - float32 [B] -, next_action uint8 [B, N]).
    ``next_state`` float32 [M, N, F] and ``reward`` float32 [M, N] are the replay buffer, read in place through ``index`` (int64 [B];
    None: every env-step in order); ``noise`` float32 [B, N, 2] the gumbel noise of the N picks of every row.  ``tgt_actor``: one
    module for all agents, or a sequence of N - agent k's pick then comes from ``tgt_actor[k]`` (ddpg.py:282-284;
    mdr_maddpg_target_agents).  Nothing is differentiated."""
    what = "maddpg_target"
    N = int(reward.shape[1]) if reward.dim() == 2 else 0
    per_agent = _is_seq(tgt_actor)
    why = _agents_refusal(tgt_actor, tgt_critic, N) if per_agent else _refusal(tgt_actor, tgt_critic, N)
    if why:
        raise ValueError("%s: %s" % (what, why))
    tgt_actors = list(tgt_actor) if per_agent else None
    if per_agent:
        tgt_actor = tgt_actors[0]
    dev, M, ld, B = _check_steps(tgt_actor, next_state, index, N, what)
    L.whole(reward, torch.float32, M * N, dev, what, "reward")
    L.whole(noise, torch.float32, B * N * 2, dev, what, "noise")
    cdesc = L.mlp_desc(L.fc_layers(tgt_critic))
    adescs = L.mlp_descs([L.fc_layers(m) for m in tgt_actors]) if per_agent else L.mlp_desc(L.fc_layers(tgt_actor))
    y = torch.empty(B, dtype=torch.float32, device=dev)
    next_q = torch.empty(B, dtype=torch.float32, device=dev)
    next_action = torch.empty((B, N), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _target_launch(adescs, cdesc, next_state, ld, reward, index, B, N, agent, noise, y, next_q, next_action, L.stream(dev), tau, gamma,
                       max_workgroups)
    return y, next_q, next_action


def joint_q_loss_backward(actor, critic, state: torch.Tensor, action: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None,
                          want_q: bool = False, max_workgroups: int = 0):
    """``F.mse_loss(critic(cat(states, actions)), y)`` and ``backward()`` of ddpg.py:312-327: fills ``p.grad`` of the six parameters of
    ``critic`` (allocated where None, overwritten otherwise) and returns the loss (0-dim device tensor) [and q, float32 [B]].  ``state``
    float32 [M, N, F] and ``action`` int64 [M, N] are the replay buffer, read in place through ``index``; ``y`` float32 [B]
    (``maddpg_target``'s) in minibatch order.  ``actor`` gives F (it is not evaluated)."""
    what = "joint_q_loss_backward"
    N = int(action.shape[1]) if action.dim() == 2 else 0
    why = _refusal(actor, critic, N)
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev, M, ld, B = _check_steps(actor, state, index, N, what)
    L.whole(action, torch.int64, M * N, dev, what, "action")
    L.whole(y, torch.float32, B, dev, what, "y")
    adesc, cdesc = L.mlp_desc(L.fc_layers(actor)), L.mlp_desc(L.fc_layers(critic))
    _, c_floats, nbytes = _sizes(adesc, cdesc, N, B, max_workgroups)
    flat = L.flat_grad(critic, c_floats, dev)
    ws = L.workspace(dev, nbytes)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    q = torch.empty(B, dtype=torch.float32, device=dev) if want_q else None
    with torch.cuda.device(dev):
        _critic_launch(cdesc, state, ld, action, index, B, N, y, ws, flat, loss, q, L.stream(dev), max_workgroups)
    L.publish(L.mlp_params(L.fc_layers(critic)), flat, L.KEEP)
    return (loss, q) if want_q else loss


def actor_loss_backward(actor, critic, state: torch.Tensor, action: torch.Tensor, agent: int, noise: torch.Tensor, tau: float = 1.0,
                        pse: float = PSE, index: Optional[torch.Tensor] = None, want_q: bool = False, max_workgroups: int = 0):
    """The actor's loss of ddpg.py:331-339 for agent ``agent`` and ``backward()``: fills ``p.grad`` of the six parameters of ``actor``
    and returns the loss (0-dim device tensor) [and Q float32 [B], logits float32 [B, 2]].  ``noise`` float32 [B, 2]: the gumbel
    noise of the row's sample.  The critic is read, its ``.grad`` is not touched."""
    what = "actor_loss_backward"
    N = int(action.shape[1]) if action.dim() == 2 else 0
    why = _refusal(actor, critic, N)
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev, M, ld, B = _check_steps(actor, state, index, N, what)
    L.whole(action, torch.int64, M * N, dev, what, "action")
    L.whole(noise, torch.float32, B * 2, dev, what, "noise")
    adesc, cdesc = L.mlp_desc(L.fc_layers(actor)), L.mlp_desc(L.fc_layers(critic))
    a_floats, _, nbytes = _sizes(adesc, cdesc, N, B, max_workgroups)
    flat = L.flat_grad(actor, a_floats, dev)
    ws = L.workspace(dev, nbytes)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    q = torch.empty(B, dtype=torch.float32, device=dev) if want_q else None
    logits = torch.empty((B, 2), dtype=torch.float32, device=dev) if want_q else None
    with torch.cuda.device(dev):
        _actor_launch(adesc, cdesc, state, ld, action, index, B, N, agent, noise, ws, flat, loss, q, logits, L.stream(dev), tau, pse, max_workgroups)
    L.publish(L.mlp_params(L.fc_layers(actor)), flat, L.KEEP)
    return (loss, q, logits) if want_q else loss


class JointReplayBuffer(L.RingBuffer):
    """The N per-agent ``Buffer``s of ddpg.py:208-213, 250-262 (which always hold the same env-steps) as one ring over env-steps on
    ``device`` (``_learner.RingBuffer``): ``state`` / ``next_state`` [capacity, N, F], ``action`` int64 [capacity, N], ``reward``
    [capacity, N].  ``push``: ``n`` env-steps at once, ``state`` / ``next_state`` [n, N, F], ``action`` / ``reward`` [n, N];
    ``push_batch``: the dict of ``collect_maddpg_transitions`` (``state`` [T + 1, E, N, F]), stored in (t, env) order."""

    def __init__(self, capacity: int, nb_agents: int, num_state: int, device):
        if int(capacity) <= 0 or int(nb_agents) <= 0 or int(num_state) <= 0:
            raise ValueError("JointReplayBuffer: capacity, nb_agents and num_state must be positive")
        self.nb_agents = int(nb_agents)
        super().__init__(capacity, (self.nb_agents,), num_state, device)

    def _rows(self, n, state, next_state, action, reward):
        s3, s2 = (n, self.nb_agents, self.num_state), (n, self.nb_agents)
        if state.shape != s3 or next_state.shape != s3 or action.shape != s2 or reward.shape != s2:
            raise ValueError("JointReplayBuffer.push: state / next_state [n, %d, %d], action and reward [n, %d]" % (s3[1], s3[2], s3[1]))
        return state, next_state, action, reward

    def sample(self, batch_size: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``batch_size`` distinct positions (int64 on the device) drawn uniformly from the filled part WITHOUT replacement, as
        ``np.random.choice(total_num, size=batch_size, replace=False)`` draws them (ddpg.py:268)."""
        if int(batch_size) > self._len:
            raise ValueError("JointReplayBuffer.sample: %d env-steps asked of %d" % (int(batch_size), self._len))
        return torch.randperm(self._len, generator=generator, device=self.device)[:int(batch_size)]


class MADDPGLearner:
    """``MADDPG`` of agents/ddpg.py without the acting half: the actor, the critic, a target of each loaded from it (ddpg.py:79-91),
    the joint replay buffer and the two optimisers; ``store`` and ``update``.  ``shared=True`` (default): one actor, one critic and
    one target of each for all agents (module docstring).  ``shared=False``: the reference's per-agent networks (ddpg.py:200-213) -
    ``actor`` and ``critic`` are sequences of ``nb_agents`` modules of one shape each, and every agent has its own targets and its
    own two optimisers.  Either way ``actors``, ``critics``, ``tgt_actors``, ``tgt_critics``, ``actor_optimizers`` and
    ``critic_optimizers`` are lists of ``nb_agents`` (shared: every entry the one shared object); ``actor``, ``critic``,
    ``tgt_actor``, ``tgt_critic``, ``actor_optimizer`` and ``critic_optimizer`` are the shared objects, and None when unshared.

    ``backend="hip"``: target, both losses and both gradients from the kernels (ValueError for networks they refuse); ``"torch"``: the
    reference's expressions under autograd - the comparator and the fallback; ``"auto"``: the kernels where ``supported()`` holds
    and the minibatch has ``AUTO_MIN_ROWS`` to ``AUTO_MAX_ROWS`` rows (where they measured faster), torch otherwise.  ``optimizer``: called as ``optimizer(params, lr)`` for
    each network; with ``mdr_amd.optim.FusedAdam`` every clip + Adam is one ``step(max_grad_norm=0.5)`` and the last step of each net
    in an ``update()`` carries the target blend (``target=..., tau=soft_tau``).  Unshared nets take ONE step each per ``update()``:
    critic a's blend rides on critic a's step (nobody reads ``tgt_critics[a]`` afterwards), the actors' blends never ride - every
    later agent of the same update reads ``tgt_actors[a]`` as the previous update left it - and follow the loop.  ``"auto"`` resolves
    to torch for unshared nets (``AUTO_UNSHARED`` above).

    ``sampler="philox"``: ``draws()`` is one launch of mdr_maddpg_draws keyed by (seed, training_step) instead of N ``randperm`` and
    one ``exponential_`` under a ``torch.Generator`` (``"torch"``, the default) - other draws of the same laws, on every backend.
    ``graph=True`` (implies ``sampler="philox"``; needs ``optimizer=FusedAdam`` and networks the kernels take): every ``update()`` is
    replayed from one captured graph (graph_update.MADDPGUpdateGraph) and gives the bits of the eager ``sampler="philox"`` update;
    ``graph_captures`` counts the captures.

    ``agent_steps="batched"`` (``shared=False``, ``backend="hip"``, ``optimizer=FusedAdam``, no graph; ValueError otherwise): the N
    agents go through every stage of an update TOGETHER instead of one after the other - mdr_maddpg_target_all,
    mdr_maddpg_critic_grad_all, one ``optim.step_nets`` over the N critics (each critic's blend riding on it), mdr_maddpg_actor_grad_all,
    one ``step_nets`` over the N actors, the actors' blends - about ten launches with N times the workgroups each, and the bits of
    the default ``"sequential"``: with unshared nets agent a's steps read nothing another agent's steps of the same update write
    (DESIGN.md).  ``before_step`` is called for the N critics after the critics' gradients and for the N actors after the actors'.
    The gradients are slices of one [N, G] buffer per kind; the nets' tensors must keep their addresses (``load_network_dict``
    does).  The attribute may be changed between updates; optimisers at different step counts (a heterogeneous
    ``load_network_dict``) take their steps one by one for that update."""

    MAX_GRAD_NORM = 0.5      # ddpg.py:157, 163

    def __init__(self, actor, critic, nb_agents: int, lr_actor: float, lr_critic: float, gamma: float = 0.99, soft_tau: float = 0.01,
                 gumbel_tau: float = 1.0, batch_size: int = 64, buffer_capacity: int = 524288, backend: str = "auto",
                 optimizer=torch.optim.Adam, shared: bool = True, sampler: Optional[str] = None, graph: bool = False,
                 agent_steps: str = "sequential"):
        L.check_backend(backend)
        if agent_steps not in ("sequential", "batched"):
            raise ValueError("agent_steps must be 'sequential' or 'batched'")
        if agent_steps == "batched":      # decided before anything touches the GPU
            for bad, why in ((shared, "shared=False (the steps of agents that share their nets depend on each other)"),
                             (backend != "hip", "backend='hip'"), (optimizer is not FusedAdam, "optimizer=FusedAdam"),
                             (graph, "graph=False (capturing the batched update is not offered)")):
                if bad:
                    raise ValueError("MADDPGLearner(agent_steps='batched') needs " + why)
        self.agent_steps = agent_steps
        self.sampler, self.graph = L.check_sampler(sampler, graph), bool(graph)
        self.shared, self.nb_agents = bool(shared), int(nb_agents)
        N = self.nb_agents
        if self.shared:
            if backend == "hip":
                L.require(_refusal(actor, critic, nb_agents), "MADDPGLearner")
            actors, critics = [actor], [critic]
        else:
            if not _is_seq(actor) or not _is_seq(critic) or len(actor) != N or len(critic) != N:
                raise ValueError("MADDPGLearner(shared=False): actor and critic must be sequences of nb_agents = %d modules" % N)
            actors, critics = list(actor), list(critic)
        if any(L.fc_layers(m) is None for m in actors + critics):
            raise ValueError("MADDPGLearner: actor and critic need the reference's Linear-ReLU-Linear-ReLU-Linear stack (DDPGNetworkMLP)")
        for nets, what in ((actors, "actor"), (critics, "critic")):
            shape = [lin.weight.shape for lin in L.fc_layers(nets[0])]
            for k, m in enumerate(nets):
                if [lin.weight.shape for lin in L.fc_layers(m)] != shape:
                    raise ValueError("MADDPGLearner(shared=False): agent %d's %s has another shape than agent 0's" % (k, what))
        if not self.shared and backend == "hip":
            L.require(_agents_refusal(actors, critics[0], N), "MADDPGLearner")
            for k in range(N):
                L.require(_refusal(actors[k], critics[k], N), "MADDPGLearner")
        fa, fc = L.fc_layers(actors[0]), L.fc_layers(critics[0])
        dev = fa[0].weight.device
        self.num_state = fa[0].in_features
        if fc[0].in_features != self.nb_agents * (self.num_state + 2):
            raise ValueError("MADDPGLearner: the critic must read nb_agents * (num_state + 2) inputs")
        tgt_actors = [DDPGNetworkMLP(self.num_state, fa[2].out_features, fa[0].out_features).to(dev) for _ in actors]
        tgt_critics = [DDPGNetworkMLP(fc[0].in_features, fc[2].out_features, fc[0].out_features).to(dev) for _ in critics]
        for tgt, net in list(zip(tgt_actors, actors)) + list(zip(tgt_critics, critics)):
            for t, s in zip(tgt.fc, net.fc):
                if t.weight.shape != s.weight.shape:
                    raise ValueError("MADDPGLearner: both hidden layers of a net have the same width in the reference")
                t.weight.data.copy_(s.weight.data)
                t.bias.data.copy_(s.bias.data)
        self.gamma, self.soft_tau, self.gumbel_tau = float(gamma), float(soft_tau), float(gumbel_tau)
        self.lr_actor, self.lr_critic = lr_actor, lr_critic
        self.batch_size, self.backend = int(batch_size), backend
        self.buffer = JointReplayBuffer(buffer_capacity, self.nb_agents, self.num_state, dev)
        actor_optimizers = [optimizer(m.parameters(), lr_actor) for m in actors]
        critic_optimizers = [optimizer(m.parameters(), lr_critic) for m in critics]
        rep = N if self.shared else 1      # shared: every entry of the lists is the one shared object
        self.actors, self.critics, self.tgt_actors, self.tgt_critics = actors * rep, critics * rep, tgt_actors * rep, tgt_critics * rep
        self.actor_optimizers, self.critic_optimizers = actor_optimizers * rep, critic_optimizers * rep
        one = (lambda lst: lst[0]) if self.shared else (lambda lst: None)
        self.actor, self.critic, self.tgt_actor, self.tgt_critic = one(actors), one(critics), one(tgt_actors), one(tgt_critics)
        self.actor_optimizer, self.critic_optimizer = one(actor_optimizers), one(critic_optimizers)
        self.training_step = 0
        # optional callable(learner, "critic" | "actor", agent): after a backward, before its clip and step - the gradient to look at
        # is critics[agent]'s or actors[agent]'s
        self.before_step = None
        self.graph_captures = 0
        self._graph = None
        self._batched = None
        if agent_steps == "batched":
            self._batched_state()      # the gradients' slices exist before any update, whichever form takes it
        if self.graph:
            why = graph_update.refusal(backend, self.sampler, actor_optimizers + critic_optimizers, self.uses_kernels(max(self.batch_size, 1)))
            if why:
                raise ValueError("MADDPGLearner(graph=True): " + why)

    @classmethod
    def from_config(cls, ddpg_prop: dict, actor, critic, nb_agents: int, backend: str = "auto", optimizer=torch.optim.Adam,
                    sampler: Optional[str] = None, graph: bool = False, agent_steps: str = "sequential") -> "MADDPGLearner":
        """From the reference's ``config_dict["DDPG_prop"]`` (agents/ddpg.py:60-70).  ``DDPG_shared`` (ddpg.py:214-215; absent: shared)
        false: ``actor`` and ``critic`` are the caller's lists of ``nb_agents`` modules."""
        return cls(actor, critic, nb_agents, ddpg_prop["lr_actor"], ddpg_prop["lr_critic"], gamma=ddpg_prop["gamma"],
                   soft_tau=ddpg_prop["soft_tau"], gumbel_tau=ddpg_prop["gumbel_softmax_tau"], batch_size=ddpg_prop["batch_size"],
                   buffer_capacity=ddpg_prop["buffer_capacity"], backend=backend, optimizer=optimizer,
                   shared=bool(ddpg_prop.get("DDPG_shared", True)), sampler=sampler, graph=graph, agent_steps=agent_steps)

    def uses_kernels(self, nb_rows: int) -> bool:
        if self.backend == "auto":
            if not self.shared:      # every net would have to pass (_agents_refusal and _refusal of each pair, targets too)
                return AUTO_UNSHARED
            return (_refusal(self.actor, self.critic, self.nb_agents) is None and
                    _refusal(self.tgt_actor, self.tgt_critic, self.nb_agents) is None and AUTO_MIN_ROWS <= nb_rows <= AUTO_MAX_ROWS)
        return self.backend == "hip"

    def network_dict(self) -> Dict[int, dict]:
        """The dict ``saveDDPGDict`` writes (utils.py:1165-1187): one entry per agent - the four state_dicts (keys ``net.0|2|4.*``),
        the two optimisers' and the scalars.  Shared: every entry repeats the one set."""
        return {i: {"actor_state_dict": self.actors[i].state_dict(), "actor_optimizer_state_dict": self.actor_optimizers[i].state_dict(),
                    "critic_state_dict": self.critics[i].state_dict(), "critic_optimizer_state_dict": self.critic_optimizers[i].state_dict(),
                    "tgt_actor_net_state_dict": self.tgt_actors[i].state_dict(), "tgt_critic_net_state_dict": self.tgt_critics[i].state_dict(),
                    "lr_actor": self.lr_actor, "lr_critic": self.lr_critic, "gamma": self.gamma, "soft_tau": self.soft_tau}
                for i in range(self.nb_agents)}

    def load_network_dict(self, d: Dict[int, dict]) -> None:
        """Load a ``network_dict()`` - or a dict the reference wrote - in place: the tensors keep their addresses.  Entry i goes to
        agent i's nets (shared: entry 0 to the one set); optimiser states are loaded where the entry has them."""
        if sorted(d.keys()) != list(range(self.nb_agents)):
            raise ValueError("load_network_dict: one entry per agent 0 .. %d expected" % (self.nb_agents - 1))
        for i in range(1 if self.shared else self.nb_agents):
            e = d[i]
            for net, key in ((self.actors[i], "actor_state_dict"), (self.critics[i], "critic_state_dict"),
                             (self.tgt_actors[i], "tgt_actor_net_state_dict"), (self.tgt_critics[i], "tgt_critic_net_state_dict")):
                net.load_state_dict(e[key])
            for opt, key in ((self.actor_optimizers[i], "actor_optimizer_state_dict"), (self.critic_optimizers[i], "critic_optimizer_state_dict")):
                if e.get(key) is not None:      # a copy: torch keeps tensors of the right dtype and device as they are, and a dict taken
                    opt.load_state_dict(copy.deepcopy(e[key]))      # from a live learner would share its Adam moments with this one

    def store(self, batch: Dict[str, torch.Tensor]) -> None:
        """``MADDPG.push`` (ddpg.py:250-262) for every env-step of a ``collect_maddpg_transitions`` dict."""
        self.buffer.push_batch(batch)

    def draws(self, seed: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The minibatches and the noise of this update, from one ``torch.Generator`` seeded by (seed, training_step) - the same on
        every backend: index int64 [N, B] (agent a's fresh minibatch, ddpg.py:307), and in ONE draw the gumbel noise
        ``-log(Exp(1))`` (what ``F.gumbel_softmax`` draws) float32 [N, B, N + 1, 2]: [a, :, :N] for the target actor's picks of agent
        a's update, [a, :, N] for the actor's own sample."""
        dev, N, B = self.buffer.device, self.nb_agents, self.batch_size
        if self.sampler == "philox":      # one launch by (seed, training_step): graph_update.maddpg_draws
            return graph_update.maddpg_draws(N, B, len(self.buffer), seed, self.training_step, dev)
        gen = L.seeded_generator(seed, self.training_step, dev)
        index = torch.stack([self.buffer.sample(B, gen) for _ in range(N)])
        noise = -torch.empty((N, B, N + 1, 2), dtype=torch.float32, device=dev).exponential_(generator=gen).log()
        return index, noise[:, :, :N].contiguous(), noise[:, :, N].contiguous()

    @staticmethod
    def _hard(logits: torch.Tensor, noise: torch.Tensor, tau: float) -> torch.Tensor:
        """``F.gumbel_softmax(logits, tau, hard=True)`` on the given gumbel noise: y_hard - y_soft.detach() + y_soft."""
        y_soft = ((logits + noise) / tau).softmax(-1)
        index = y_soft.max(-1, keepdim=True)[1]
        y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
        return y_hard - y_soft.detach() + y_soft

    def _kernels(self):
        """(sizes, target launch, critic launch, actor launch) of the calls ``critic_backward`` and ``actor_backward`` make, this
        learner's fixed arguments bound: what a captured graph runs on its static buffers (graph_update.MADDPGUpdateGraph)."""
        return (_sizes, partial(_target_launch, tau=self.gumbel_tau, gamma=self.gamma), _critic_launch,
                partial(_actor_launch, tau=self.gumbel_tau, pse=PSE))

    def _capture(self):
        """Capture the graph of one update without replaying it; every net, the moments and every counter are what they were."""
        self._graph = graph_update.MADDPGUpdateGraph(self)
        self.graph_captures += 1
        return self._graph

    def update_target(self) -> None:
        """ddpg.py:167-174: to = soft_tau * from + (1 - soft_tau) * to over both pairs of nets."""
        n = 1 if self.shared else self.nb_agents
        for tgt, net in list(zip(self.tgt_actors[:n], self.actors[:n])) + list(zip(self.tgt_critics[:n], self.critics[:n])):
            L.blend(L.mlp_params(tgt.fc), L.mlp_params(net.fc), self.soft_tau)

    def _step(self, opt, net, blend_target) -> None:
        """clip_grad_norm_(0.5) and the optimiser step of one net; ``blend_target``: the target net whose blend rides on this step
        (a FusedAdam's; None: no blend)."""
        if blend_target is not None:
            L.clip_and_step(opt, net.parameters(), self.MAX_GRAD_NORM, target=L.mlp_params(blend_target.fc), tau=self.soft_tau)
        else:
            L.clip_and_step(opt, net.parameters(), self.MAX_GRAD_NORM)

    def critic_backward(self, agent: int, index: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """Target, mse loss and backward of the critic for agent ``agent`` on the env-steps at ``index``: fills the ``.grad`` of
        ``critics[agent]``.  Unshared: every agent's next action from ITS OWN target actor (ddpg.py:282-284), the value from
        ``tgt_critics[agent]``."""
        buf, N = self.buffer, self.nb_agents
        critic, tgt_critic = self.critics[agent], self.tgt_critics[agent]
        if self.uses_kernels(int(index.shape[0])):
            y, _, _ = maddpg_target(self.tgt_actor if self.shared else self.tgt_actors, tgt_critic, buf.next_state, buf.reward, agent, noise,
                                    self.gumbel_tau, self.gamma, index=index)
            return joint_q_loss_backward(self.actors[agent], critic, buf.state, buf.action, y, index=index)
        B = int(index.shape[0])
        state, next_state = buf.state[index], buf.next_state[index]
        action = F.one_hot(buf.action[index].clamp(max=1), 2).to(torch.float32)
        with torch.no_grad():
            if self.shared:
                logits = self.tgt_actor(next_state)
            else:
                logits = torch.stack([self.tgt_actors[k](next_state[:, k]) for k in range(N)], 1)
            next_action = self._hard(logits, noise, self.gumbel_tau)
            next_q = tgt_critic(torch.cat((next_state.reshape(B, -1), next_action.reshape(B, -1)), 1)).squeeze(1)
            target_value = buf.reward[index][:, agent] + self.gamma * next_q
        critic_value = critic(torch.cat((state.reshape(B, -1), action.reshape(B, -1)), 1)).squeeze(1)
        loss = F.mse_loss(critic_value, target_value, reduction="mean")
        self.critic_optimizers[agent].zero_grad()
        loss.backward()
        return loss.detach()

    def actor_backward(self, agent: int, index: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """The actor's loss and backward for agent ``agent``: fills the ``.grad`` of ``actors[agent]``, through ``critics[agent]``."""
        buf = self.buffer
        actor, critic = self.actors[agent], self.critics[agent]
        if self.uses_kernels(int(index.shape[0])):
            return actor_loss_backward(actor, critic, buf.state, buf.action, agent, noise, self.gumbel_tau, PSE, index=index)
        B = int(index.shape[0])
        state = buf.state[index]
        action = F.one_hot(buf.action[index].clamp(max=1), 2).to(torch.float32)
        logits = actor(state[:, agent])
        action_ = self._hard(logits, noise, self.gumbel_tau)
        action = torch.cat((action[:, :agent], action_[:, None], action[:, agent + 1:]), 1)
        for p in critic.parameters():      # the reference lets this backward write the critic's .grad and zeroes it later
            p.requires_grad_(False)
        try:
            actor_loss = -critic(torch.cat((state.reshape(B, -1), action.reshape(B, -1)), 1)).squeeze(1).mean()
            loss = actor_loss + PSE * torch.pow(logits, 2).mean()
            self.actor_optimizers[agent].zero_grad()
            loss.backward()
        finally:
            for p in critic.parameters():
                p.requires_grad_(True)
        return loss.detach()

    def _batched_state(self) -> dict:
        """What the batched update keeps: the four host arrays of descriptors, the parameter lists, and one [N, G] gradient buffer per
        kind whose slice a is ``_mdr_flat_grad`` of agent a's module - what ``publish`` and the sequential calls write too."""
        if self._batched is not None:
            return self._batched
        if self.shared or self.backend != "hip" or self.graph:
            raise ValueError("MADDPGLearner: agent_steps='batched' needs shared=False, backend='hip' and graph=False")
        N, B, dev = self.nb_agents, self.batch_size, self.buffer.device
        lib = nat.load()
        descs = [L.mlp_descs([L.fc_layers(m) for m in nets]) for nets in (self.actors, self.critics, self.tgt_actors, self.tgt_critics)]
        a_floats, c_floats, _ = _sizes(descs[0][0], descs[1][0], N, B)
        nbytes = L.sized(int(lib.mdr_maddpg_workspace_bytes_all(C.byref(descs[0][0]), C.byref(descs[1][0]), N, B, 0)), "MADDPGLearner",
                         "mdr_maddpg_workspace_bytes_all")
        flat_a = torch.empty((N, a_floats), dtype=torch.float32, device=dev)
        flat_c = torch.empty((N, c_floats), dtype=torch.float32, device=dev)
        for a in range(N):
            self.actors[a]._mdr_flat_grad, self.critics[a]._mdr_flat_grad = flat_a[a], flat_c[a]
        self._batched = dict(descs=descs, nbytes=nbytes, flat_a=flat_a, flat_c=flat_c,
                             a_params=[L.mlp_params(m.fc) for m in self.actors], c_params=[L.mlp_params(m.fc) for m in self.critics],
                             tc_params=[L.mlp_params(m.fc) for m in self.tgt_critics],
                             ta_all=[p for m in self.tgt_actors for p in L.mlp_params(m.fc)],
                             a_all=[p for m in self.actors for p in L.mlp_params(m.fc)])
        return self._batched

    def _update_batched(self, seed: int) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """``update`` with the agents side by side (class docstring): the stages of the unshared loop below, each over all N agents."""
        if len(self.buffer) < self.batch_size:
            return None
        st, buf, N, B = self._batched_state(), self.buffer, self.nb_agents, self.batch_size
        adescs, cdescs, tgt_adescs, tgt_cdescs = st["descs"]
        dev = buf.device
        index, noise_t, noise_a = self.draws(seed)
        _, _, ld, _ = _check_steps(self.actors[0], buf.state, index[0], N, "MADDPGLearner.update")
        y = torch.empty((N, B), dtype=torch.float32, device=dev)
        next_action = torch.empty((N, B, N), dtype=torch.uint8, device=dev)
        c_loss = torch.empty(N, dtype=torch.float32, device=dev)
        a_loss = torch.empty(N, dtype=torch.float32, device=dev)
        ws = L.workspace(dev, st["nbytes"])
        with torch.cuda.device(dev):
            stream = L.stream(dev)
            _target_all_launch(tgt_adescs, tgt_cdescs, buf.next_state, ld, buf.reward, index, B, N, noise_t, y, None, next_action, stream,
                               self.gumbel_tau, self.gamma)
            _critic_all_launch(cdescs, buf.state, ld, buf.action, index, B, N, y, ws, st["flat_c"], c_loss, None, stream)
        self._publish_and_step("critic", self.critics, self.critic_optimizers, st["c_params"], st["flat_c"], st["tc_params"])
        with torch.cuda.device(dev):      # the actors' step reads the stepped critics
            _actor_all_launch(adescs, cdescs, buf.state, ld, buf.action, index, B, N, noise_a, ws, st["flat_a"], a_loss, None, None,
                              L.stream(dev), self.gumbel_tau, PSE)
        self._publish_and_step("actor", self.actors, self.actor_optimizers, st["a_params"], st["flat_a"], None)
        L.blend(st["ta_all"], st["a_all"], self.soft_tau)      # the N actors' blends: after every step, as the loop has them
        self.training_step += 1
        return a_loss, c_loss

    def _publish_and_step(self, which, nets, optimizers, params, flat, blend_targets) -> None:
        """``.grad`` of the N nets from the slices of ``flat``, the N ``before_step`` calls, then clip + Adam [+ blend] of all N: one
        ``step_nets``, or the nets' own steps where their optimisers do not go together."""
        N = self.nb_agents
        for a in range(N):
            L.publish(params[a], flat[a], L.KEEP)
        if self.before_step is not None:
            for a in range(N):
                self.before_step(self, which, a)
        if nets_refusal(optimizers) is None:
            step_nets(optimizers, self.MAX_GRAD_NORM, targets=blend_targets, tau=self.soft_tau if blend_targets is not None else 0.0)
        else:
            for a in range(N):
                self._step(optimizers[a], nets[a], self.tgt_critics[a] if blend_targets is not None else None)

    def update(self, seed: int = 0) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """One ``MADDPG.update()`` (ddpg.py:305-339) and the ``update_target()`` train_ddpg.py:124-131 follows it with: for every agent
        in order a fresh minibatch, the critic's step, the actor's step; then one blend of both target nets.  -> (actor_loss [N],
        critic_loss [N]) as device tensors (the actor's loss includes the 1e-3 logits term), or None while the buffer holds fewer
        than ``batch_size`` env-steps."""
        if self.graph:
            return graph_update.maddpg_update(self, seed)
        if self.agent_steps == "batched":
            return self._update_batched(seed)
        if len(self.buffer) < self.batch_size:
            return None
        N = self.nb_agents
        index, noise_t, noise_a = self.draws(seed)
        fused_a, fused_c = isinstance(self.actor_optimizers[0], FusedAdam), isinstance(self.critic_optimizers[0], FusedAdam)
        a_losses, c_losses = [], []
        if not self.shared:
            # ddpg.py:305-339 literally: per agent a fresh minibatch, every agent's next action from its own target actor as the
            # PREVIOUS update left it, critic a's step, actor a's step; then the 2 N blends.  Critic a's blend may ride on its step;
            # an actor's may not - tgt_actors[a] is read by every later agent of this update
            for a in range(N):
                c_losses.append(self.critic_backward(a, index[a], noise_t[a]))
                if self.before_step is not None:
                    self.before_step(self, "critic", a)
                self._step(self.critic_optimizers[a], self.critics[a], self.tgt_critics[a] if fused_c else None)
                a_losses.append(self.actor_backward(a, index[a], noise_a[a]))
                if self.before_step is not None:
                    self.before_step(self, "actor", a)
                self._step(self.actor_optimizers[a], self.actors[a], None)
            for a in range(N):
                L.blend(L.mlp_params(self.tgt_actors[a].fc), L.mlp_params(self.actors[a].fc), self.soft_tau)
                if not fused_c:
                    L.blend(L.mlp_params(self.tgt_critics[a].fc), L.mlp_params(self.critics[a].fc), self.soft_tau)
            self.training_step += 1
            return torch.stack(a_losses), torch.stack(c_losses)
        for a in range(N):
            last = a == N - 1
            c_losses.append(self.critic_backward(a, index[a], noise_t[a]))
            if self.before_step is not None:
                self.before_step(self, "critic", a)
            self._step(self.critic_optimizer, self.critic, self.tgt_critic if last and fused_c else None)
            a_losses.append(self.actor_backward(a, index[a], noise_a[a]))
            if self.before_step is not None:
                self.before_step(self, "actor", a)
            self._step(self.actor_optimizer, self.actor, self.tgt_actor if last and fused_a else None)
        for tgt, net, done in ((self.tgt_actor, self.actor, fused_a), (self.tgt_critic, self.critic, fused_c)):
            if not done:      # the blend did not ride on this net's last step
                L.blend(L.mlp_params(tgt.fc), L.mlp_params(net.fc), self.soft_tau)
        self.training_step += 1
        return torch.stack(a_losses), torch.stack(c_losses)


class GreedyDDPGActor:
    """``DDPGAgent.act`` (agents/rl_controllers.py): the argmax of the actor's logits, in the shape ``deploy_policy`` takes through
    its duck-typed branch - ``.sample(rows, seed, step, action=None, step_dev=None)`` -> uint8 actions.  ``backend="torch"`` (default):
    a torch forward and a compare; ``"hip"``: the greedy form of ``FusedMLPActor`` - forward and argmax in one kernel (ValueError for a
    net it does not take); it honours ``step_dev``, which a greedy pick does not read.  ``"hip-bf16x3"``: that form with
    ``precision="bf16x3"`` (one shared net only).  ``actor``: one module, or a sequence of N (unshared networks): row e N + k is
    agent k's and goes through ``actor[k]`` - N torch forwards, or ``FusedMLPActors`` (fp32 only: ValueError with "hip-bf16x3").
    One shared net on a hip backend also has ``sample_env`` - the actions from the env's compact state, no observation rows -
    which ``deploy_policy(..., observe_act=True)`` takes where ``observe_supported(env)`` holds."""

    def __init__(self, actor, backend: str = "torch"):
        if backend not in ("torch", "hip", "hip-bf16x3"):
            raise ValueError("backend must be 'torch', 'hip' or 'hip-bf16x3'")
        self.actor, self.backend = (list(actor) if _is_seq(actor) else actor), backend
        self.per_agent = _is_seq(actor)
        self._fused = self._a_prob = None
        if backend != "torch":
            from .mlp_actor import FusedMLPActor, FusedMLPActors
            if self.per_agent and backend == "hip-bf16x3":
                raise ValueError("GreedyDDPGActor(backend='hip-bf16x3'): one net per agent acts in fp32 only (FusedMLPActors)")
            kind = FusedMLPActors if self.per_agent else FusedMLPActor
            why = kind.refusal(self.actor)
            if why:
                raise ValueError("GreedyDDPGActor(backend=%r): %s" % (backend, why))
            self._fused = kind(self.actor, greedy=True) if backend == "hip" else kind(self.actor, greedy=True, precision="bf16x3")

    @torch.no_grad()
    def sample(self, rows: torch.Tensor, seed: int = 0, step: int = 0, action: Optional[torch.Tensor] = None, step_dev=None) -> torch.Tensor:
        if self._fused is not None:
            if self._a_prob is None or self._a_prob.numel() != rows.shape[0] or self._a_prob.device != rows.device:
                self._a_prob = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)      # kept: a captured step allocates nothing
            return self._fused.sample(rows, seed, step, step_dev=step_dev, action=action, a_prob=self._a_prob)[0]
        if self.per_agent:
            N = len(self.actor)
            per = rows.view(rows.shape[0] // N, N, rows.shape[1])
            logits = torch.stack([self.actor[k](per[:, k]) for k in range(N)], 1).view(rows.shape[0], 2)
        else:
            logits = self.actor(rows)
        act = logits[:, 1] > logits[:, 0]      # argmax keeps the first maximum
        if action is None:
            return act.to(torch.uint8)
        action.copy_(act)
        return action

    def observe_supported(self, env) -> bool:
        """Can ``sample_env`` serve ``env``?  One shared net behind ``backend="hip"`` or ``"hip-bf16x3"`` and
        ``FusedMLPActor.observe_supported(env)``.  Decided on the host."""
        return self._fused is not None and not self.per_agent and self._fused.observe_supported(env)

    @torch.no_grad()
    def sample_env(self, env, seed: int = 0, step: int = 0, action: Optional[torch.Tensor] = None, step_dev=None) -> torch.Tensor:
        """``sample(env.obs_vector("rows").view(E * N, 51), ...)`` without the rows (``FusedMLPActor.sample_env``): the same actions,
        bit for bit.  ValueError for a list of nets, ``backend="torch"`` or an env the kernel does not cover."""
        if self._fused is None or self.per_agent:
            raise ValueError("GreedyDDPGActor.sample_env: one shared net with backend='hip' or 'hip-bf16x3' only")
        why = self._fused._observe_refusal(env)
        if why:
            raise ValueError("GreedyDDPGActor.sample_env: " + why)
        A = env.nb_envs * env.nb_houses
        if self._a_prob is None or self._a_prob.numel() != A or self._a_prob.device != env.device:
            self._a_prob = torch.empty(A, dtype=torch.float32, device=env.device)      # kept: a captured step allocates nothing
        return self._fused.sample_env(env, seed, step, step_dev=step_dev, action=action, a_prob=self._a_prob)[0]


def train_maddpg(env, learner: MADDPGLearner, nb_steps: int, update_every: int = 1, random_steps: int = 0, seed: int = 0,
                 actor_backend: str = "torch", observe_act: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The loop of train_ddpg.py:95-131 on a batched env (reset by the caller): every iteration one ``collect_maddpg_transitions``
    step of all envs (uniformly random actions while the 1-based step is below ``random_steps``, the actor's gumbel sample after), ``store``, and
    after every ``update_every``-th step from ``random_steps`` on one ``update()`` (which ends with the target blend).
    ``actor_backend`` is ``collect_maddpg_transitions``': "hip" acts through ``FusedMLPActor``, which reads the actor's weights in
    place and so sees every update; "hip-bf16x3" is its bf16x3 precision (a shared actor only).  ``observe_act`` is
    ``collect_maddpg_transitions``' too: the acting steps through ``FusedMLPActor.sample_env``, the same transitions bit for bit.
    -> (actor losses [n, N], critic losses [n, N]) of the updates that ran, on the device."""
    from .rollout import collect_maddpg_transitions
    a_losses, c_losses = [], []
    for t in range(int(nb_steps)):
        step = t + 1      # train_ddpg.py:96-97, 124-127: random while step < random_steps, learn from step >= random_steps on
        batch = collect_maddpg_transitions(env, learner.actor if getattr(learner, "shared", True) else learner.actors, 1, random_steps_left=max(int(random_steps) - step, 0),
                                           seed=(int(seed) * 1000003 + t) & (2 ** 63 - 1), actor_backend=actor_backend,
                                           observe_act=observe_act)
        learner.store(batch)
        if step >= int(random_steps) and step % int(update_every) == 0:
            out = learner.update(seed=seed)
            if out is not None:
                a_losses.append(out[0])
                c_losses.append(out[1])
    dev, N = learner.buffer.device, learner.nb_agents
    empty = torch.empty((0, N), dtype=torch.float32, device=dev)
    return (torch.stack(a_losses) if a_losses else empty), (torch.stack(c_losses) if c_losses else empty.clone())
