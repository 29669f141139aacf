"""PPO's update step on the GPU (include/mdr_policy.h: mdr_ppo_actor_grad, mdr_ppo_critic_grad).

The other half of the reference's train_ppo.py: ``PPO.update`` (agents/ppo.py:139-188) on the transitions ``collect_ppo_rollout``
leaves on the device.  Per minibatch the reference evaluates critic and actor, forms F.mse_loss and the clipped surrogate, calls
``backward()`` twice, clips both gradients and takes two Adam steps.  Here forward, loss and backward of one network are ONE HIP
kernel on the matrix cores in exact fp32 (plus a small reduction): ``critic_loss_backward`` / ``actor_loss_backward`` fill the
``.grad`` of an ``ActorMLP`` / ``CriticMLP``, torch keeps the gradient clipping and the optimiser (``optimizer=FusedAdam``, optim.py: one launch for both).  ``PPOLearner`` is the loop.
Nothing on the call path synchronises with the host.  Networks of 65..128 input features - observations with message columns -
take the same kernels' wide instantiations with ``wide=True`` (mdr_ppo_actor_grad_wide, mdr_ppo_critic_grad_wide).
``precision="bf16x3"`` (opt-in, narrow networks only) takes the same chain with its five matrix products on the bf16 matrix cores, every
operand split into a bf16 head and tail (mdr_ppo_actor_grad_bf16x3, mdr_ppo_critic_grad_bf16x3; profiles/ppo_update_bf16_README.md).
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _learner as L
from . import _native as nat
from . import graph_update

MAX_STATE, MAX_HIDDEN = 64, 128      # the kernels' limits (include/mdr_policy.h: mdr_mlp_t)
# backend="auto": the kernels from this many minibatch rows on (profiles/ppo_update_README.md: where they measured faster than autograd)
AUTO_MIN_ROWS = 1
# wide=True: 65..128 input features (the observations with message columns) through the mdr_*_wide entry points, which have the
# narrow ones' argument lists.  Their backend="auto" threshold is measured on its own (profiles/wide_update_README.md).
MAX_STATE_WIDE = 128
AUTO_MIN_ROWS_WIDE = 1
_WIDE = L.WIDE
# precision="bf16x3": the entry points with the five matrix products as three bf16 products each (csrc/mdr_ppo_grad_bf16.hip); the
# argument lists, the limits and the size functions of the fp32 ones
PRECISIONS = ("fp32", "bf16x3")
_BF16X3 = {"mdr_ppo_actor_grad": "mdr_ppo_actor_grad_bf16x3", "mdr_ppo_critic_grad": "mdr_ppo_critic_grad_bf16x3"}


def check_precision(precision: str, wide: bool = False, what: str = "precision") -> str:
    """``precision`` if it is one of ``PRECISIONS`` and the entry points asked for have it (ValueError otherwise)."""
    if precision not in PRECISIONS:
        raise ValueError("%s must be 'fp32' or 'bf16x3'" % what)
    if precision == "bf16x3" and wide:
        raise ValueError("precision='bf16x3' covers the narrow entry points only (F <= %d): not with wide=True" % MAX_STATE)
    return precision


def _entry(lib, name: str, wide: bool, precision: str):
    if precision == "bf16x3":
        name = _BF16X3[name]
        return getattr(lib, name), name
    return L.fn(lib, name, wide)


def refusal(net, num_out: Optional[int] = None, max_state: int = MAX_STATE, wide: bool = False, precision: str = "fp32") -> Optional[str]:
    """Why the kernels do not take ``net`` (None: they do).  ``max_state``: the input width of the head asked for.  ``wide``: the
    wide entry points' limits - ``MAX_STATE_WIDE`` input features and the LDS fit, the message saying which of the two failed.
    ``precision="bf16x3"``: the narrow limits, every shape inside them (ValueError with ``wide=True`` or an unknown precision)."""
    check_precision(precision, wide)
    return L.mlp_refusal(net, (1, 2) if num_out is None else (num_out,), MAX_STATE_WIDE if wide else max_state, MAX_HIDDEN, wide)


_refusal = refusal      # (its name before mappo and dqn called it)


def supported(net, wide: bool = False, precision: str = "fp32") -> bool:
    """Do the gradient kernels take this network?  An ``ActorMLP`` / ``CriticMLP`` of two hidden layers with F <= 64 input features,
    hidden layers of at most 128 units and 2 (actor) or 1 (critic) outputs, float32 on the GPU.  ``wide=True``: the wide entry
    points, F <= 128 where the LDS layout fits (hidden 100-100: every F; 128-128: F <= 100).  ``precision="bf16x3"``: the narrow
    limits again - those kernels refuse no shape inside them."""
    return refusal(net, wide=wide, precision=precision) is None


def _actor_launch(desc, state, ld, action, old_prob, index, B, advantage, workspace, flat, loss, ratio, stream, clip_param, max_workgroups=0,
                  wide=False, precision="fp32") -> None:
    """mdr_ppo_actor_grad[_wide | _bf16x3] on checked tensors, under the device of ``state``: the eager call and the captured one."""
    lib = nat.load()
    call, name = _entry(lib, "mdr_ppo_actor_grad", wide, precision)
    nat.check(lib, None, call(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, L.ptr(action), L.ptr(old_prob), L.ptr(advantage),
                              C.c_float(clip_param), max_workgroups, L.ptr(workspace), L.ptr(flat), L.ptr(loss), L.ptr(ratio), stream), name)


def _critic_launch(desc, state, ld, action, target, index, B, workspace, flat, loss, value, adv, stream, max_workgroups=0, wide=False,
                   precision="fp32") -> None:
    """mdr_ppo_critic_grad[_wide | _bf16x3] on checked tensors; ``action`` is not read (mappo's joint launch, with the same list, reads it)."""
    lib = nat.load()
    call, name = _entry(lib, "mdr_ppo_critic_grad", wide, precision)
    nat.check(lib, None, call(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, L.ptr(target), max_workgroups, L.ptr(workspace), L.ptr(flat),
                              L.ptr(loss), L.ptr(value), L.ptr(adv), stream), name)


def actor_loss_backward(actor, state: torch.Tensor, action: torch.Tensor, old_prob: torch.Tensor, advantage: torch.Tensor,
                        clip_param: float = 0.2, index: Optional[torch.Tensor] = None, want_ratio: bool = False, max_workgroups: int = 0,
                        wide: bool = False, precision: str = "fp32"):
    """The clipped surrogate of agents/ppo.py:153-169 and ``backward()`` in one kernel: fills ``p.grad`` of the six parameters of
    ``actor`` (allocated where None, overwritten otherwise) and returns the loss (0-dim device tensor) [and the ratios, float32 [B]].
    ``state`` float32 [M, F] (any row stride >= F), ``action`` int64 [M], ``old_prob`` float32 [M]: the transition buffer, read in
    place through ``index`` (int64 [B] on the device; None: every row in order, B = M); ``advantage`` float32 [B] in minibatch order.
    ``wide=True``: up to 128 input features (``supported(actor, wide=True)``).  ``precision="bf16x3"``: the matrix products as three
    bf16 products of split operands each, fp32 accumulation, everything else as it is (include/mdr_policy.h has the contract)."""
    what = "actor_loss_backward"
    why = refusal(actor, 2, wide=wide, precision=precision)
    if why:
        raise ValueError("%s: %s" % (what, why))
    fc = L.fc_layers(actor)
    dev, M, ld, B = L.check_rows(fc, state, index, what)
    L.whole(action, torch.int64, M, dev, what, "action")
    L.whole(old_prob, torch.float32, M, dev, what, "old_prob")
    L.whole(advantage, torch.float32, B, dev, what, "advantage")
    if not 0.0 <= float(clip_param) < 1.0:
        raise ValueError("%s: clip_param must lie in [0, 1)" % what)
    desc = L.mlp_desc(fc)
    floats, nbytes = L.mlp_sizes(desc, B, max_workgroups, wide)
    flat = L.flat_grad(actor, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ratio = torch.empty(B, dtype=torch.float32, device=dev) if want_ratio else None
    with torch.cuda.device(dev):
        _actor_launch(desc, state, ld, action, old_prob, index, B, advantage, L.workspace(dev, nbytes), flat, loss, ratio, L.stream(dev),
                      clip_param, max_workgroups, wide, precision)
    L.publish(L.mlp_params(fc), flat, L.KEEP)
    return (loss, ratio) if want_ratio else loss


def critic_loss_backward(critic, state: torch.Tensor, target: torch.Tensor, index: Optional[torch.Tensor] = None,
                         max_workgroups: int = 0, wide: bool = False, precision: str = "fp32") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """F.mse_loss(Gt, V) of agents/ppo.py:148-150, 180 and ``backward()`` in one kernel: fills ``p.grad`` of ``critic`` and returns
    (loss 0-dim, value float32 [B], advantage float32 [B] = target - value, the detached delta the actor's loss takes).
    ``target`` float32 [M] is read through ``index`` like ``state``.  ``wide=True``: up to 128 input features.  ``precision``: as
    ``actor_loss_backward``."""
    what = "critic_loss_backward"
    why = refusal(critic, 1, wide=wide, precision=precision)
    if why:
        raise ValueError("%s: %s" % (what, why))
    fc = L.fc_layers(critic)
    dev, M, ld, B = L.check_rows(fc, state, index, what)
    L.whole(target, torch.float32, M, dev, what, "target")
    desc = L.mlp_desc(fc)
    floats, nbytes = L.mlp_sizes(desc, B, max_workgroups, wide)
    flat = L.flat_grad(critic, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev)
    adv = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _critic_launch(desc, state, ld, None, target, index, B, L.workspace(dev, nbytes), flat, loss, value, adv, L.stream(dev), max_workgroups, wide,
                       precision)
    L.publish(L.mlp_params(fc), flat, L.KEEP)
    return loss, value, adv


class PPOLearner:
    """``PPO.update`` (agents/ppo.py:139-188) on the dict ``collect_ppo_rollout`` returns.

    ``backend="hip"``: both losses and gradients from the kernels (ValueError for networks they refuse); ``"torch"``: the
    reference's expressions under autograd - the comparator and the fallback; ``"auto"``: the kernels where ``supported()`` holds
    for both networks and the minibatch has at least ``AUTO_MIN_ROWS`` rows, torch otherwise.  ``optimizer``: called as
    ``optimizer(params, lr)`` for each network; an optimiser that is a ``mdr_amd.optim.FusedAdam`` clips and steps in one launch
    (``.grad`` then keeps the unclipped gradient), any other one is stepped after ``clip_grad_norm_``.  ``wide=True``: the wide
    entry points, so networks of up to 128 input features (both message flags on: 121) take the kernels, eager or ``graph=True``;
    ``"auto"`` then takes them from ``AUTO_MIN_ROWS_WIDE`` minibatch rows on.  ``precision="bf16x3"``: every kernel call of this
    learner in that precision, eager or ``graph=True``; opt-in only (``"auto"`` never picks it by itself), it needs the kernels:
    ValueError for a network they refuse, with ``backend="torch"`` and with ``wide=True``."""

    def __init__(self, actor, critic, lr_actor: float, lr_critic: float, clip_param: float = 0.2, max_grad_norm: float = 0.5,
                 ppo_update_time: int = 10, batch_size: int = 256, backend: str = "auto", optimizer=torch.optim.Adam,
                 sampler: Optional[str] = None, graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False,
                 precision: str = "fp32"):
        L.check_backend(backend)
        self.wide = bool(wide)
        self.precision = check_precision(precision, self.wide, "%s: precision" % type(self).__name__)
        sampler = L.check_sampler(sampler, graph)
        if backend == "hip":
            L.require(refusal(actor, 2, wide=self.wide) or refusal(critic, 1, wide=self.wide), "PPOLearner")
        if self.precision == "bf16x3":
            self._require_bf16x3(actor, critic, backend)
        self.actor, self.critic = actor, critic
        self.clip_param, self.max_grad_norm = float(clip_param), float(max_grad_norm)
        self.ppo_update_time, self.batch_size = int(ppo_update_time), int(batch_size)
        self.backend = backend
        self.actor_optimizer = optimizer(actor.parameters(), lr_actor)
        self.critic_optimizer = optimizer(critic.parameters(), lr_critic)
        self.training_step = 0
        self.before_clip = None      # optional callable(learner): runs after both backward passes of a minibatch, before the clipping
        # sampler="philox": the minibatch indices from csrc/mdr_minibatch.hip by (seed, epoch) instead of a torch.Generator;
        # graph=True: every epoch of an update replayed from one captured graph per batch shape (graph_update.py)
        self.sampler, self.graph, self.graph_max_minibatches = sampler, bool(graph), int(graph_max_minibatches)
        self.graph_captures = 0
        self._graphs: Dict[tuple, object] = {}
        if self.graph:
            why = graph_update.refusal(backend, sampler, (self.actor_optimizer, self.critic_optimizer), self.uses_kernels(max(self.batch_size, 1)))
            if why:
                raise ValueError("%s(graph=True): %s" % (type(self).__name__, why))

    def _require_bf16x3(self, actor, critic, backend: str) -> None:
        """``precision="bf16x3"`` exists in the kernels alone, for the networks they take."""
        if backend == "torch":
            raise ValueError("%s(precision='bf16x3'): the precision of the HIP kernels, not of backend='torch'" % type(self).__name__)
        why = refusal(actor, 2, precision="bf16x3") or refusal(critic, 1, precision="bf16x3")
        if why:
            raise ValueError("%s(precision='bf16x3'): %s" % (type(self).__name__, why))

    @classmethod
    def from_config(cls, ppo_prop: dict, actor, critic, backend: str = "auto", optimizer=torch.optim.Adam, sampler: Optional[str] = None,
                    graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False, precision: str = "fp32") -> "PPOLearner":
        """From the reference's ``config_dict["PPO_prop"]`` (agents/ppo.py:34-40)."""
        return cls(actor, critic, ppo_prop["lr_actor"], ppo_prop["lr_critic"], clip_param=ppo_prop["clip_param"],
                   max_grad_norm=ppo_prop["max_grad_norm"], ppo_update_time=ppo_prop["ppo_update_time"],
                   batch_size=ppo_prop["batch_size"], backend=backend, optimizer=optimizer, sampler=sampler, graph=graph,
                   graph_max_minibatches=graph_max_minibatches, wide=wide, precision=precision)

    def uses_kernels(self, nb_rows: int) -> bool:
        if self.precision == "bf16x3":      # asked for by name and checked at construction: never autograd at another precision
            return True
        if self.backend == "auto":
            return (refusal(self.actor, 2, wide=self.wide) is None and refusal(self.critic, 1, wide=self.wide) is None
                    and nb_rows >= (AUTO_MIN_ROWS_WIDE if self.wide else AUTO_MIN_ROWS))
        return self.backend == "hip"

    def minibatches(self, nb_transitions: int, seed: int, epoch: int) -> List[torch.Tensor]:
        """The index tensors (int64, on the actor's device) of one epoch (``_learner.minibatches`` under this learner's sampler)."""
        return L.minibatches(next(self.actor.parameters()).device, nb_transitions, self.batch_size, self.sampler, seed, epoch)

    def critic_backward(self, state, action, target, index):
        """The critic's kernel call of one minibatch -> (loss, value, advantage); MAPPOLearner's takes the joint input."""
        return critic_loss_backward(self.critic, state, target, index=index, wide=self.wide, precision=self.precision)

    def _critic_kernel(self):
        """(sizes, launch) of the call ``critic_backward`` makes, this learner's fixed arguments bound: what a captured graph runs on
        its static buffers (graph_update.PPOUpdateGraph).  MAPPOLearner's is the joint one, with the same argument lists."""
        return partial(L.mlp_sizes, wide=self.wide), partial(_critic_launch, wide=self.wide, precision=self.precision)

    def _actor_kernel(self):
        """The same of the actor's call."""
        return partial(L.mlp_sizes, wide=self.wide), partial(_actor_launch, clip_param=self.clip_param, wide=self.wide, precision=self.precision)

    def _capture(self, shape):
        """Capture the graph of one epoch over a batch of ``shape`` = (T, A, F) without replaying it; parameters, moments and every
        counter are what they were."""
        T, A, F = (int(x) for x in shape)
        g = graph_update.PPOUpdateGraph(self, T, A, F)
        self._graphs[(T, A, F, self.ppo_update_time, self.batch_size)] = g
        self.graph_captures += 1
        return g

    def critic_input(self, state, action, index) -> torch.Tensor:
        """The critic's input rows of one minibatch on the torch backend."""
        return state[index]

    def step_minibatch(self, state, action, old_prob, target, index) -> Tuple[torch.Tensor, torch.Tensor]:
        """One minibatch of agents/ppo.py:146-188: critic, actor with the critic's advantage, gradient clipping on each network, both
        optimiser steps.  The arguments are the whole flattened buffers; ``index`` picks the minibatch.  -> (actor loss, critic loss)."""
        if self.uses_kernels(int(index.shape[0])):
            value_loss, _, advantage = self.critic_backward(state, action, target, index)
            action_loss = actor_loss_backward(self.actor, state, action, old_prob, advantage, self.clip_param, index=index, wide=self.wide,
                                              precision=self.precision)
        else:
            Gt_index = target[index].view(-1, 1)
            V = self.critic(self.critic_input(state, action, index))
            advantage = (Gt_index - V).detach()
            action_prob = self.actor(state[index]).gather(1, action[index].view(-1, 1))
            ratio = action_prob / old_prob[index].view(-1, 1)
            surr1 = ratio * advantage
            surr2 = torch.clamp(ratio, 1 - self.clip_param, 1 + self.clip_param) * advantage
            action_loss = -torch.min(surr1, surr2).mean()
            self.actor_optimizer.zero_grad()
            action_loss.backward()
            value_loss = F.mse_loss(Gt_index, V)
            self.critic_optimizer.zero_grad()
            value_loss.backward()
            action_loss, value_loss = action_loss.detach(), value_loss.detach()
        if self.before_clip is not None:
            self.before_clip(self)
        L.clip(self.actor_optimizer, self.actor.parameters(), self.max_grad_norm)      # both clips before both steps
        L.clip(self.critic_optimizer, self.critic.parameters(), self.max_grad_norm)
        L.step(self.actor_optimizer, self.max_grad_norm)
        L.step(self.critic_optimizer, self.max_grad_norm)
        self.training_step += 1
        return action_loss, value_loss

    def update(self, batch: Dict[str, torch.Tensor], seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``ppo_update_time`` epochs over ``batch`` (``state`` [T+1, A, F], ``action``, ``a_prob``, ``return`` [T, A]): the states are
        ``batch["state"][:-1]`` flattened to [T A, F] and read in place, Gt is ``batch["return"]``.  -> (mean actor loss, mean critic
        loss - device tensors -, number of minibatches).  ``graph=True``: the same launches replayed from a captured graph, the same
        bits as the eager ``sampler="philox"`` update."""
        if self.graph:
            done = graph_update.ppo_update(self, batch, seed)
            if done is not None:      # None: an empty batch, nothing to replay
                return done
        states = batch["state"]
        T = states.shape[0] - 1
        state = states[:T].reshape(-1, states.shape[-1])      # a view: the first T slabs of a contiguous buffer
        action = batch["action"].reshape(-1)
        old_prob = batch["a_prob"].reshape(-1)
        target = batch["return"].reshape(-1)
        return L.mean_losses(state.device, 2, self.ppo_update_time, lambda epoch: self.minibatches(state.shape[0], seed, epoch),
                             lambda index: self.step_minibatch(state, action, old_prob, target, index))
