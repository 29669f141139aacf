"""MAPPO's update step on the GPU (include/mdr_policy.h: mdr_mappo_critic_grad, mdr_ppo_actor_grad).

``MAPPO.update`` (agents/mappo.py:60-119) on the transitions ``collect_ppo_rollout(..., with_others_actions=True)`` leaves on the
device.  Its actor step is PPO's line for line (mappo.py:92-110), so ``ppo.actor_loss_backward`` serves it unchanged; its critic is
``Critic(num_state + nb_agents - 1)`` on ``torch.cat((state, others_actions))`` (mappo.py:21, 87).  ``joint_critic_loss_backward`` is
forward, F.mse_loss and backward of that critic in ONE HIP kernel, which gathers the other agents' actions of a transition from the
``action`` buffer while it stages the tile (they are the transition's env-mates): the int64 [T, E N, N - 1] ``others_actions`` tensor is
neither read nor needed.  ``MAPPOLearner`` is the loop; clipping and Adam stay torch.  Nothing on the call path synchronises.

Places that leave the reference's text on purpose:

* ``MAPPO.update`` runs ONE ``Gt`` recursion over its flat buffer (mappo.py:68-74), which train_mappo.py:86 fills step by step with the
  agents interleaved: within an episode the return of agent k at step t continues with agent k + 1's reward of the SAME step (agent
  N - 1's with agent 0's of the next), so one step's N rewards are discounted against each other N times per step.  Here
  ``batch["return"]`` is ``rollout.discounted_returns`` along time for each agent's own rewards, as in PPO - what the reference
  computes when the same transitions are stored agent by agent.  ``MAPPOLearner.update`` itself takes ``batch["return"]`` as given:
  fed the reference's storage-order ``Gt`` it reproduces the reference's update (tests/test_learner_golden.py pins both).
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from typing import Dict, Optional, Tuple

import torch

from . import _learner as L
from . import _native as nat
from . import ppo
from .ppo import PPOLearner

MAX_JOINT, MAX_HIDDEN = 128, ppo.MAX_HIDDEN      # the joint head's limits (include/mdr_policy.h: mdr_mappo_critic_grad)
# backend="auto": the kernels from this many minibatch rows on (profiles/mappo_update_README.md: where they measured faster than the
# torch backend)
AUTO_MIN_ROWS = 1
# the same for wide=True (profiles/wide_update_README.md)
AUTO_MIN_ROWS_WIDE = 1


def _joint_refusal(critic, num_state: int, wide: bool = False) -> Optional[str]:
    """Why the joint-input kernel does not take ``critic`` over states of ``num_state`` features (None: it does).  ``wide``: the
    LDS fit of mdr_mappo_critic_grad_wide's layout; the 128 joint inputs are the limit of both."""
    why = ppo.refusal(critic, 1, max_state=MAX_JOINT)
    if why:
        return why
    J = critic.fc[0].in_features
    nb_agents = J - int(num_state) + 1
    if num_state < 1 or nb_agents < 1:
        return "a critic of %d inputs over states of %d features leaves no whole number of other agents" % (J, num_state)
    if L.fn(nat.load(), "mdr_mappo_critic_grad_floats", wide)[0](C.byref(L.mlp_desc(L.fc_layers(critic))), nb_agents) < 0:
        return ("%d joint inputs with hidden layers of %d and %d units do not fit the kernel's LDS layout"
                % (J, critic.fc[0].out_features, critic.fc[1].out_features))
    return None


def supported(critic, num_state: int, wide: bool = False) -> bool:
    """Does the joint-input kernel take this critic over states of ``num_state`` features?  A ``CriticMLP(num_state + N - 1)`` of two
    hidden layers with at most 128 joint inputs, hidden layers of at most 128 units and an LDS layout that fits (hidden 100-100: up
    to 100 inputs; 128-128: up to 68; 64-64: 128), float32 on the GPU.  ``wide=True``: the wide entry point, whose layout fits hidden
    100-100 up to 128 inputs and 128-128 up to 100.  More than 128 joint inputs stay refused either way: states of 121 features (both
    message flags on) leave room for 8 agents, and the reference's 20 agents make 140 inputs."""
    return _joint_refusal(critic, num_state, wide=wide) is None


def gather_others(action: torch.Tensor, nb_agents: int, index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``others_actions`` (train_mappo.py:79-84) of the transitions ``index`` (None: all) from the flat ``action`` buffer of
    ``collect_ppo_rollout`` (the agent index runs fastest): [B, nb_agents - 1], entry k of transition j the action of agent k
    (k < j % N) or k + 1 of the same env-step.  What the torch backend takes when the batch carries no ``others_actions``."""
    N = int(nb_agents)
    j = torch.arange(action.numel(), device=action.device) if index is None else index
    a = (j % N)[:, None]
    k = torch.arange(N - 1, device=action.device)[None, :]
    return action.reshape(-1)[(j[:, None] - a) + k + (k >= a).to(k.dtype)]


def _joint_sizes(desc, nb_rows: int, max_workgroups: int = 0, *, nb_agents: int, wide: bool = False) -> Tuple[int, int]:
    """(floats of the flat gradient, bytes of workspace) of the joint critic's call over ``nb_rows`` rows."""
    lib = nat.load()
    return (int(L.fn(lib, "mdr_mappo_critic_grad_floats", wide)[0](C.byref(desc), nb_agents)),
            int(L.fn(lib, "mdr_mappo_critic_workspace_bytes", wide)[0](C.byref(desc), nb_agents, nb_rows, max_workgroups)))


def _joint_critic_launch(desc, state, ld, action, target, index, B, workspace, flat, loss, value, adv, stream, max_workgroups=0, *, nb_agents,
                         wide=False) -> None:
    """mdr_mappo_critic_grad[_wide] on checked tensors (``action``: the whole buffer, one element per transition), under the device
    of ``state``: the eager call and the captured one.  The argument list of ``ppo._critic_launch``."""
    lib = nat.load()
    call, name = L.fn(lib, "mdr_mappo_critic_grad", wide)
    nat.check(lib, None, call(C.byref(desc), L.ptr(state), ld, L.ptr(action), action.numel(), nb_agents, L.ptr(index), B, L.ptr(target),
                              max_workgroups, L.ptr(workspace), L.ptr(flat), L.ptr(loss), L.ptr(value), L.ptr(adv), stream), name)


def joint_critic_loss_backward(critic, state: torch.Tensor, action: torch.Tensor, target: torch.Tensor, nb_agents: Optional[int] = None,
                               index: Optional[torch.Tensor] = None, max_workgroups: int = 0,
                               wide: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """F.mse_loss(Gt, V) of agents/mappo.py:85-88, 113 with V = critic(cat(state, others_actions)) and ``backward()`` in one kernel:
    fills ``p.grad`` of ``critic`` and returns (loss 0-dim, value float32 [B], advantage float32 [B] = target - value, detached).
    ``state`` float32 [M, F] (any row stride >= F), ``action`` int64 [M], ``target`` float32 [M]: the transition buffer in
    ``collect_ppo_rollout``'s flat order (M a multiple of ``nb_agents``, default ``critic.fc[0].in_features - F + 1``), read in place
    through ``index`` (int64 [B] on the device; None: every row in order).  The others' actions are gathered from ``action``.
    ``wide=True``: the wide entry point's LDS fit (``supported(critic, F, wide=True)``); more than 128 joint inputs stay refused."""
    what = "joint_critic_loss_backward"
    if state.dim() != 2:
        raise ValueError("%s: state must be a float32 [M, F] tensor" % what)
    F_len = int(state.shape[1])
    fc = L.fc_layers(critic)
    if nb_agents is None and fc is not None:
        nb_agents = fc[0].in_features - F_len + 1
    why = _joint_refusal(critic, F_len, wide=wide)
    if why:
        raise ValueError("%s: %s" % (what, why))
    if int(nb_agents) != fc[0].in_features - F_len + 1:
        raise ValueError("%s: a critic of %d inputs over states of %d features has %d agents, not %d"
                         % (what, fc[0].in_features, F_len, fc[0].in_features - F_len + 1, nb_agents))
    N = int(nb_agents)
    dev, M, ld, B = L.check_rows(fc, state, index, what, num_state=F_len)
    if M % N:
        raise ValueError("%s: a buffer of %d transitions is no whole number of env-steps of %d agents" % (what, M, N))
    L.whole(action, torch.int64, M, dev, what, "action")
    L.whole(target, torch.float32, M, dev, what, "target")
    desc = L.mlp_desc(fc)
    floats, nbytes = _joint_sizes(desc, B, max_workgroups, nb_agents=N, wide=wide)
    flat = L.flat_grad(critic, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev)
    adv = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _joint_critic_launch(desc, state, ld, action, target, index, B, L.workspace(dev, nbytes), flat, loss, value, adv, L.stream(dev),
                             max_workgroups, nb_agents=N, wide=wide)
    L.publish(L.mlp_params(fc), flat, L.KEEP)
    return loss, value, adv


class MAPPOLearner(PPOLearner):
    """``MAPPO.update`` (agents/mappo.py:60-119) on the dict ``collect_ppo_rollout(..., with_others_actions=True)`` returns.

    The critic is ``CriticMLP(F + nb_agents - 1)``: the number of agents comes from its width.  ``backend="hip"``: the joint critic
    kernel, then ``ppo.actor_loss_backward`` with its advantage (ValueError for networks they refuse); ``"torch"``: the reference's
    expressions under autograd on ``torch.cat((state[index], others[index].float()), 1)`` - the comparator and the fallback;
    ``"auto"``: the kernels where they take both networks and the minibatch has at least ``AUTO_MIN_ROWS`` rows.  ``wide=True``:
    the wide entry points for both networks - states of up to 128 features and a joint input of up to 128 (F = 121 with at most 8
    agents; F = 121 with 20 agents is 140 inputs and stays refused); ``"auto"`` then counts from ``AUTO_MIN_ROWS_WIDE`` rows."""

    def __init__(self, actor, critic, lr_actor: float, lr_critic: float, clip_param: float = 0.2, max_grad_norm: float = 0.5,
                 ppo_update_time: int = 10, batch_size: int = 256, backend: str = "auto", optimizer=torch.optim.Adam,
                 sampler: Optional[str] = None, graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False):
        L.check_backend(backend)
        afc, cfc = L.fc_layers(actor), L.fc_layers(critic)
        if afc is None or cfc is None:
            raise ValueError("MAPPOLearner: actor and critic must be Linear-ReLU-Linear-ReLU-Linear (an `fc` ModuleList of three biased Linear layers)")
        self.num_state = afc[0].in_features
        self.nb_agents = cfc[0].in_features - self.num_state + 1
        if self.nb_agents < 1:
            raise ValueError("MAPPOLearner: the critic takes num_state + nb_agents - 1 = %d + N - 1 inputs, not %d" % (self.num_state, cfc[0].in_features))
        if backend == "hip":
            L.require(ppo.refusal(actor, 2, wide=wide) or _joint_refusal(critic, self.num_state, wide=wide), "MAPPOLearner")
        # the base class checks PPO's critic (over the state alone) for "hip": this one's is checked above
        super().__init__(actor, critic, lr_actor, lr_critic, clip_param=clip_param, max_grad_norm=max_grad_norm, ppo_update_time=ppo_update_time,
                         batch_size=batch_size, backend="auto" if backend == "hip" else backend, optimizer=optimizer, sampler=sampler, graph=graph,
                         graph_max_minibatches=graph_max_minibatches, wide=wide)
        self.backend = backend
        self._others = None      # the batch's others_actions [M, N - 1] during an update of the torch backend, where it has them

    @classmethod
    def from_config(cls, mappo_prop: dict, actor, critic, backend: str = "auto", optimizer=torch.optim.Adam, sampler: Optional[str] = None,
                    graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False) -> "MAPPOLearner":
        """From the reference's ``config_dict["MAPPO_prop"]`` (agents/mappo.py:23-29)."""
        return cls(actor, critic, mappo_prop["lr_actor"], mappo_prop["lr_critic"], clip_param=mappo_prop["clip_param"],
                   max_grad_norm=mappo_prop["max_grad_norm"], ppo_update_time=mappo_prop["ppo_update_time"],
                   batch_size=mappo_prop["batch_size"], backend=backend, optimizer=optimizer, sampler=sampler, graph=graph,
                   graph_max_minibatches=graph_max_minibatches, wide=wide)

    def uses_kernels(self, nb_rows: int) -> bool:
        if self.backend == "auto":
            return (ppo.refusal(self.actor, 2, wide=self.wide) is None and _joint_refusal(self.critic, self.num_state, wide=self.wide) is None
                    and nb_rows >= (AUTO_MIN_ROWS_WIDE if self.wide else AUTO_MIN_ROWS))
        return self.backend == "hip"

    def critic_backward(self, state, action, target, index):
        return joint_critic_loss_backward(self.critic, state, action, target, nb_agents=self.nb_agents, index=index, wide=self.wide)

    def _critic_kernel(self):
        return (partial(_joint_sizes, nb_agents=self.nb_agents, wide=self.wide),
                partial(_joint_critic_launch, nb_agents=self.nb_agents, wide=self.wide))

    def critic_input(self, state, action, index) -> torch.Tensor:
        """agents/mappo.py:87: torch.cat((state[index], others_actions[index]), dim=1)."""
        others = self._others[index] if self._others is not None else gather_others(action, self.nb_agents, index)
        return torch.cat((state[index], others.float()), 1)

    def update(self, batch: Dict[str, torch.Tensor], seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``ppo_update_time`` epochs over ``batch`` as ``PPOLearner.update``; ``batch["others_actions"]`` [T, A, N - 1] is optional and
        read by the torch backend alone (without it that backend gathers each minibatch's from ``batch["action"]``)."""
        A = int(batch["action"].shape[1])
        if A % self.nb_agents:
            raise ValueError("MAPPOLearner.update: %d agents per step are no whole number of envs of %d agents (the critic's width)" % (A, self.nb_agents))
        if int(batch["state"].shape[-1]) != self.num_state:
            raise ValueError("MAPPOLearner.update: states of %d features, the actor takes %d" % (batch["state"].shape[-1], self.num_state))
        if self.backend != "hip" and "others_actions" in batch:
            others = batch["others_actions"]
            if others.shape[-1] != self.nb_agents - 1:
                raise ValueError("MAPPOLearner.update: others_actions of %d columns, the critic's width asks for %d" % (others.shape[-1], self.nb_agents - 1))
            self._others = others.reshape(-1, self.nb_agents - 1)
        try:
            return super().update(batch, seed)
        finally:
            self._others = None
