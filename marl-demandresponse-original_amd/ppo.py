"""PPO's update step on the GPU (include/mdr_policy.h: mdr_ppo_actor_grad, mdr_ppo_critic_grad).

The other half of the reference's train_ppo.py: ``PPO.update`` (agents/ppo.py:139-188) on the transitions ``collect_ppo_rollout``
leaves on the device.  Per minibatch the reference evaluates critic and actor, forms F.mse_loss and the clipped surrogate, calls
``backward()`` twice, clips both gradients and takes two Adam steps.  Here forward, loss and backward of one network are ONE HIP
kernel on the matrix cores in exact fp32 (plus a small reduction): ``critic_loss_backward`` / ``actor_loss_backward`` fill the
``.grad`` of an ``ActorMLP`` / ``CriticMLP``, torch keeps the gradient clipping and the optimiser (``optimizer=FusedAdam``, optim.py: one launch for both).  ``PPOLearner`` is the loop.
Nothing on the call path synchronises with the host.  Networks of 65..128 input features - observations with message columns -
take the same kernels' wide instantiations with ``wide=True`` (mdr_ppo_actor_grad_wide, mdr_ppo_critic_grad_wide).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from .optim import FusedAdam

MAX_STATE, MAX_HIDDEN = 64, 128      # the kernels' limits (include/mdr_policy.h: mdr_mlp_t)
# backend="auto": the kernels from this many minibatch rows on (profiles/ppo_update_README.md: where they measured faster than autograd)
AUTO_MIN_ROWS = 1
# wide=True: 65..128 input features (the observations with message columns) through the mdr_*_wide entry points, which have the
# narrow ones' argument lists.  Their backend="auto" threshold is measured on its own (profiles/wide_update_README.md).
MAX_STATE_WIDE = 128
AUTO_MIN_ROWS_WIDE = 1
_WIDE = {"mdr_mlp_grad_floats": "mdr_mlp_wide_grad_floats", "mdr_mlp_grad_workspace_bytes": "mdr_mlp_wide_grad_workspace_bytes",
         "mdr_ppo_actor_grad": "mdr_ppo_actor_grad_wide", "mdr_ppo_critic_grad": "mdr_ppo_critic_grad_wide",
         "mdr_dqn_target": "mdr_dqn_target_wide", "mdr_dqn_grad": "mdr_dqn_grad_wide",
         "mdr_mappo_critic_grad_floats": "mdr_mappo_critic_wide_grad_floats",
         "mdr_mappo_critic_workspace_bytes": "mdr_mappo_critic_wide_workspace_bytes", "mdr_mappo_critic_grad": "mdr_mappo_critic_grad_wide"}


def _fn(lib, name: str, wide: bool):
    """The entry point ``name`` or, with ``wide``, its wide sibling."""
    return getattr(lib, _WIDE[name] if wide else name)


def _layers(net) -> Optional[List[nn.Linear]]:
    fc = getattr(net, "fc", None)
    if fc is None or len(fc) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in fc):
        return None
    return list(fc)


def _refusal(net, num_out: Optional[int] = None, max_state: int = MAX_STATE, wide: bool = False) -> Optional[str]:
    """Why the kernels do not take ``net`` (None: they do).  ``max_state``: the input width of the head asked for.  ``wide``: the
    wide entry points' limits - ``MAX_STATE_WIDE`` input features and the LDS fit, the message saying which of the two failed."""
    if wide:
        max_state = MAX_STATE_WIDE
    fc = _layers(net)
    if fc is None:
        return "the kernels cover Linear-ReLU-Linear-ReLU-Linear (an `fc` ModuleList of three biased Linear layers)"
    if fc[1].in_features != fc[0].out_features or fc[2].in_features != fc[1].out_features:
        return "the three layers do not chain"
    if fc[0].in_features > max_state:
        return "num_state = %d: the kernels cover at most %d input features" % (fc[0].in_features, max_state)
    if fc[0].out_features > MAX_HIDDEN or fc[1].out_features > MAX_HIDDEN:
        return "hidden layers of %d and %d units: the kernels cover at most %d" % (fc[0].out_features, fc[1].out_features, MAX_HIDDEN)
    outs = (1, 2) if num_out is None else (num_out,)
    if fc[2].out_features not in outs:
        return "%d outputs: the kernels cover an actor of 2 actions and a critic of 1 value" % fc[2].out_features
    for lin in fc:
        for p in (lin.weight, lin.bias):
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                return "parameters must be contiguous float32 tensors on the GPU"
    if wide and nat.load().mdr_mlp_wide_grad_floats(C.byref(_desc(net))) < 0:
        return ("%d input features with hidden layers of %d and %d units do not fit the kernel's LDS layout"
                % (fc[0].in_features, fc[0].out_features, fc[1].out_features))
    return None


def supported(net, wide: bool = False) -> bool:
    """Do the gradient kernels take this network?  An ``ActorMLP`` / ``CriticMLP`` of two hidden layers with F <= 64 input features,
    hidden layers of at most 128 units and 2 (actor) or 1 (critic) outputs, float32 on the GPU.  ``wide=True``: the wide entry
    points, F <= 128 where the LDS layout fits (hidden 100-100: every F; 128-128: F <= 100)."""
    return _refusal(net, wide=wide) is None


def _params(net) -> List[torch.Tensor]:
    fc = _layers(net)
    return [fc[0].weight, fc[0].bias, fc[1].weight, fc[1].bias, fc[2].weight, fc[2].bias]


def _desc(net) -> nat.MdrMlp:
    fc = _layers(net)
    ptr = [C.c_void_p(p.data_ptr()) for p in _params(net)]
    return nat.MdrMlp(C.sizeof(nat.MdrMlp), fc[0].in_features, fc[0].out_features, fc[1].out_features, fc[2].out_features, *ptr)


_workspaces: Dict[torch.device, torch.Tensor] = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[dev] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    return ws


def _flat_grad(net, lib, desc, floats: Optional[int] = None, wide: bool = False) -> torch.Tensor:
    """The flat gradient buffer the kernels write, kept with the module; the six ``.grad`` are views of it (assigned where a
    parameter has none or another tensor of its own, which is then overwritten by a copy after the call)."""
    params = _params(net)
    flat = getattr(net, "_mdr_flat_grad", None)
    n = int(_fn(lib, "mdr_mlp_grad_floats", wide)(C.byref(desc))) if floats is None else int(floats)
    if flat is None or flat.numel() != n or flat.device != params[0].device:
        flat = torch.empty(n, dtype=torch.float32, device=params[0].device)
        net._mdr_flat_grad = flat
    return flat


def _publish(net, flat: torch.Tensor) -> None:
    off = 0
    for p in _params(net):
        view = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
        if p.grad is None:
            p.grad = view
        elif p.grad.data_ptr() != view.data_ptr():
            p.grad.copy_(view)


def _check_rows(net, state, index, what, num_state: Optional[int] = None):
    fc = _layers(net)
    dev = fc[0].weight.device
    width = fc[0].in_features if num_state is None else num_state      # of the state rows (the joint critic's input is wider)
    if state.dim() != 2 or state.shape[1] != width or state.dtype != torch.float32 or state.device != dev:
        raise ValueError("%s: state must be a float32 [M, %d] tensor on %s" % (what, width, dev))
    F_len, M = int(state.shape[1]), int(state.shape[0])
    if (F_len > 1 and state.stride(1) != 1) or (M > 1 and state.stride(0) < F_len):
        raise ValueError("%s: state rows need unit inner stride and a row stride >= F" % what)
    if index is not None and (index.dtype != torch.int64 or index.dim() != 1 or index.device != dev or not index.is_contiguous()):
        raise ValueError("%s: index must be a contiguous int64 [B] tensor on the device" % what)
    ld = int(state.stride(0)) if M > 1 else F_len
    return dev, M, ld, (int(index.shape[0]) if index is not None else M)


def _whole(t, dtype, M, dev, what, name):
    if t.dtype != dtype or t.device != dev or t.numel() != M or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of %d elements on the device" % (what, name, str(dtype).replace("torch.", ""), M))
    return t


def actor_loss_backward(actor, state: torch.Tensor, action: torch.Tensor, old_prob: torch.Tensor, advantage: torch.Tensor,
                        clip_param: float = 0.2, index: Optional[torch.Tensor] = None, want_ratio: bool = False, max_workgroups: int = 0,
                        wide: bool = False):
    """The clipped surrogate of agents/ppo.py:153-169 and ``backward()`` in one kernel: fills ``p.grad`` of the six parameters of
    ``actor`` (allocated where None, overwritten otherwise) and returns the loss (0-dim device tensor) [and the ratios, float32 [B]].
    ``state`` float32 [M, F] (any row stride >= F), ``action`` int64 [M], ``old_prob`` float32 [M]: the transition buffer, read in
    place through ``index`` (int64 [B] on the device; None: every row in order, B = M); ``advantage`` float32 [B] in minibatch order.
    ``wide=True``: up to 128 input features (``supported(actor, wide=True)``)."""
    what = "actor_loss_backward"
    why = _refusal(actor, 2, wide=wide)
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev, M, ld, B = _check_rows(actor, state, index, what)
    _whole(action, torch.int64, M, dev, what, "action")
    _whole(old_prob, torch.float32, M, dev, what, "old_prob")
    _whole(advantage, torch.float32, B, dev, what, "advantage")
    if not 0.0 <= float(clip_param) < 1.0:
        raise ValueError("%s: clip_param must lie in [0, 1)" % what)
    lib = nat.load()
    desc = _desc(actor)
    flat = _flat_grad(actor, lib, desc, wide=wide)
    ws = _workspace(dev, int(_fn(lib, "mdr_mlp_grad_workspace_bytes", wide)(C.byref(desc), B, max_workgroups)))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ratio = torch.empty(B, dtype=torch.float32, device=dev) if want_ratio else None
    with torch.cuda.device(dev):
        rc = _fn(lib, "mdr_ppo_actor_grad", wide)(
            C.byref(desc), C.c_void_p(state.data_ptr()), ld, C.c_void_p(index.data_ptr()) if index is not None else None, B,
            C.c_void_p(action.data_ptr()), C.c_void_p(old_prob.data_ptr()), C.c_void_p(advantage.data_ptr()),
            C.c_float(clip_param), max_workgroups, C.c_void_p(ws.data_ptr()), C.c_void_p(flat.data_ptr()),
            C.c_void_p(loss.data_ptr()), C.c_void_p(ratio.data_ptr()) if want_ratio else None,
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    nat.check(lib, None, rc, _WIDE["mdr_ppo_actor_grad"] if wide else "mdr_ppo_actor_grad")
    _publish(actor, flat)
    return (loss, ratio) if want_ratio else loss


def critic_loss_backward(critic, state: torch.Tensor, target: torch.Tensor, index: Optional[torch.Tensor] = None,
                         max_workgroups: int = 0, wide: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """F.mse_loss(Gt, V) of agents/ppo.py:148-150, 180 and ``backward()`` in one kernel: fills ``p.grad`` of ``critic`` and returns
    (loss 0-dim, value float32 [B], advantage float32 [B] = target - value, the detached delta the actor's loss takes).
    ``target`` float32 [M] is read through ``index`` like ``state``.  ``wide=True``: up to 128 input features."""
    what = "critic_loss_backward"
    why = _refusal(critic, 1, wide=wide)
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev, M, ld, B = _check_rows(critic, state, index, what)
    _whole(target, torch.float32, M, dev, what, "target")
    lib = nat.load()
    desc = _desc(critic)
    flat = _flat_grad(critic, lib, desc, wide=wide)
    ws = _workspace(dev, int(_fn(lib, "mdr_mlp_grad_workspace_bytes", wide)(C.byref(desc), B, max_workgroups)))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev)
    adv = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _fn(lib, "mdr_ppo_critic_grad", wide)(
            C.byref(desc), C.c_void_p(state.data_ptr()), ld, C.c_void_p(index.data_ptr()) if index is not None else None, B,
            C.c_void_p(target.data_ptr()), max_workgroups, C.c_void_p(ws.data_ptr()), C.c_void_p(flat.data_ptr()),
            C.c_void_p(loss.data_ptr()), C.c_void_p(value.data_ptr()), C.c_void_p(adv.data_ptr()),
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    nat.check(lib, None, rc, _WIDE["mdr_ppo_critic_grad"] if wide else "mdr_ppo_critic_grad")
    _publish(critic, flat)
    return loss, value, adv


class PPOLearner:
    """``PPO.update`` (agents/ppo.py:139-188) on the dict ``collect_ppo_rollout`` returns.

    ``backend="hip"``: both losses and gradients from the kernels (ValueError for networks they refuse); ``"torch"``: the
    reference's expressions under autograd - the comparator and the fallback; ``"auto"``: the kernels where ``supported()`` holds
    for both networks and the minibatch has at least ``AUTO_MIN_ROWS`` rows, torch otherwise.  ``optimizer``: called as
    ``optimizer(params, lr)`` for each network; an optimiser that is a ``mdr_amd.optim.FusedAdam`` clips and steps in one launch
    (``.grad`` then keeps the unclipped gradient), any other one is stepped after ``clip_grad_norm_``.  ``wide=True``: the wide
    entry points, so networks of up to 128 input features (both message flags on: 121) take the kernels, eager or ``graph=True``;
    ``"auto"`` then takes them from ``AUTO_MIN_ROWS_WIDE`` minibatch rows on."""

    def __init__(self, actor, critic, lr_actor: float, lr_critic: float, clip_param: float = 0.2, max_grad_norm: float = 0.5,
                 ppo_update_time: int = 10, batch_size: int = 256, backend: str = "auto", optimizer=torch.optim.Adam,
                 sampler: Optional[str] = None, graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False):
        if backend not in ("auto", "hip", "torch"):
            raise ValueError("backend must be 'auto', 'hip' or 'torch'")
        self.wide = bool(wide)
        if sampler is None:
            sampler = "philox" if graph else "torch"
        if sampler not in ("torch", "philox"):
            raise ValueError("sampler must be 'torch' or 'philox'")
        if backend == "hip":
            for net, outs in ((actor, 2), (critic, 1)):
                why = _refusal(net, outs, wide=self.wide)
                if why:
                    raise ValueError("PPOLearner(backend='hip'): " + why)
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
            from . import graph_update
            why = graph_update.refusal(backend, sampler, (self.actor_optimizer, self.critic_optimizer), self.uses_kernels(max(self.batch_size, 1)))
            if why:
                raise ValueError("%s(graph=True): %s" % (type(self).__name__, why))

    @classmethod
    def from_config(cls, ppo_prop: dict, actor, critic, backend: str = "auto", optimizer=torch.optim.Adam, sampler: Optional[str] = None,
                    graph: bool = False, graph_max_minibatches: int = 1024, wide: bool = False) -> "PPOLearner":
        """From the reference's ``config_dict["PPO_prop"]`` (agents/ppo.py:34-40)."""
        return cls(actor, critic, ppo_prop["lr_actor"], ppo_prop["lr_critic"], clip_param=ppo_prop["clip_param"],
                   max_grad_norm=ppo_prop["max_grad_norm"], ppo_update_time=ppo_prop["ppo_update_time"],
                   batch_size=ppo_prop["batch_size"], backend=backend, optimizer=optimizer, sampler=sampler, graph=graph,
                   graph_max_minibatches=graph_max_minibatches, wide=wide)

    def uses_kernels(self, nb_rows: int) -> bool:
        if self.backend == "auto":
            wide = getattr(self, "wide", False)      # (subclasses with a constructor of their own have no wide: the narrow limits)
            return (_refusal(self.actor, 2, wide=wide) is None and _refusal(self.critic, 1, wide=wide) is None
                    and nb_rows >= (AUTO_MIN_ROWS_WIDE if wide else AUTO_MIN_ROWS))
        return self.backend == "hip"

    def minibatches(self, nb_transitions: int, seed: int, epoch: int) -> List[torch.Tensor]:
        """The index tensors (int64, on the actor's device) of one epoch: a permutation of the transitions drawn from a
        ``torch.Generator`` seeded by (seed, epoch), cut into ``batch_size`` pieces; the last, shorter one is kept, as
        ``BatchSampler(SubsetRandomSampler(...), batch_size, False)`` keeps it (agents/ppo.py:140-142)."""
        dev = next(self.actor.parameters()).device
        if getattr(self, "sampler", "torch") == "philox":      # (subclasses with a constructor of their own have no sampler: torch's)
            # the Feistel permutation of (seed, epoch), one launch (graph_update.permutation): another permutation, cut the same way
            from . import graph_update
            return list(torch.split(graph_update.permutation(int(nb_transitions), seed, epoch, dev), self.batch_size))
        gen = torch.Generator(device=dev)
        gen.manual_seed((int(seed) * 1000003 + int(epoch) * 7919 + 12345) & (2 ** 63 - 1))
        perm = torch.randperm(int(nb_transitions), generator=gen, device=dev)
        return list(torch.split(perm, self.batch_size))

    def critic_backward(self, state, action, target, index):
        """The critic's kernel call of one minibatch -> (loss, value, advantage); MAPPOLearner's takes the joint input."""
        return critic_loss_backward(self.critic, state, target, index=index, wide=getattr(self, "wide", False))

    # the same call for a captured graph, on raw pointers into its static buffers (graph_update.PPOUpdateGraph); MAPPOLearner's differ
    def _critic_grad_floats(self, lib, desc) -> int:
        return int(_fn(lib, "mdr_mlp_grad_floats", getattr(self, "wide", False))(C.byref(desc)))

    def _critic_workspace_bytes(self, lib, desc, nb_rows: int) -> int:
        return int(_fn(lib, "mdr_mlp_grad_workspace_bytes", getattr(self, "wide", False))(C.byref(desc), nb_rows, 0))

    def _critic_launch(self, lib, desc, state, ld, action, nb_transitions, target, index, nb_rows, workspace, grad, loss, value, adv, stream) -> int:
        return _fn(lib, "mdr_ppo_critic_grad", getattr(self, "wide", False))(C.byref(desc), state, ld, index, nb_rows, target, 0, workspace, grad,
                                                                             loss, value, adv, stream)

    def _capture(self, shape):
        """Capture the graph of one epoch over a batch of ``shape`` = (T, A, F) without replaying it; parameters, moments and every
        counter are what they were."""
        from . import graph_update
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
            action_loss = actor_loss_backward(self.actor, state, action, old_prob, advantage, self.clip_param, index=index,
                                              wide=getattr(self, "wide", False))
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
        fused_actor, fused_critic = isinstance(self.actor_optimizer, FusedAdam), isinstance(self.critic_optimizer, FusedAdam)
        if not fused_actor:
            nn.utils.clip_grad_norm_(self.actor.parameters(), self.max_grad_norm)
        if not fused_critic:
            nn.utils.clip_grad_norm_(self.critic.parameters(), self.max_grad_norm)
        if fused_actor:      # clip and step in one launch; .grad keeps the unclipped gradient (optim.py)
            self.actor_optimizer.step(max_grad_norm=self.max_grad_norm)
        else:
            self.actor_optimizer.step()
        if fused_critic:
            self.critic_optimizer.step(max_grad_norm=self.max_grad_norm)
        else:
            self.critic_optimizer.step()
        self.training_step += 1
        return action_loss, value_loss

    def update(self, batch: Dict[str, torch.Tensor], seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``ppo_update_time`` epochs over ``batch`` (``state`` [T+1, A, F], ``action``, ``a_prob``, ``return`` [T, A]): the states are
        ``batch["state"][:-1]`` flattened to [T A, F] and read in place, Gt is ``batch["return"]``.  -> (mean actor loss, mean critic
        loss - device tensors -, number of minibatches).  ``graph=True``: the same launches replayed from a captured graph, the same
        bits as the eager ``sampler="philox"`` update."""
        if getattr(self, "graph", False):
            from . import graph_update
            done = graph_update.ppo_update(self, batch, seed)
            if done is not None:      # None: an empty batch, nothing to replay
                return done
        states = batch["state"]
        T = states.shape[0] - 1
        state = states[:T].reshape(-1, states.shape[-1])      # a view: the first T slabs of a contiguous buffer
        action = batch["action"].reshape(-1)
        old_prob = batch["a_prob"].reshape(-1)
        target = batch["return"].reshape(-1)
        n = state.shape[0]
        a_sum = torch.zeros((), dtype=torch.float32, device=state.device)
        c_sum = torch.zeros((), dtype=torch.float32, device=state.device)
        count = 0
        for epoch in range(self.ppo_update_time):
            for index in self.minibatches(n, seed, epoch):
                a_loss, c_loss = self.step_minibatch(state, action, old_prob, target, index)
                a_sum += a_loss
                c_sum += c_loss
                count += 1
        return a_sum / max(count, 1), c_sum / max(count, 1), count
