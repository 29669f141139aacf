"""TarMAC-PPO's update step on the GPU (include/mdr_policy.h: mdr_tarmac_ppo_actor_grad).

The other half of the reference's train_tarmacPPO.py: ``TarmacPPO.update`` (agents/tarmac_ppo.py:152-207) on the transitions
``collect_tarmac_rollout`` leaves on the device.  Per minibatch of stored env-steps the reference evaluates the centralised critic and
the TarMAC actor, forms the value loss and the clipped surrogate, calls ``backward()`` twice, clips both gradients and takes two
Adam steps - the actor's before the critic's.  ``actor_loss_backward`` is the actor's forward, loss and backward as hand-written HIP
kernels on the matrix cores in exact fp32 around the two banded-attention kernels (csrc/mdr_tarmac_ppo_grad.hip, no library GEMM);
it fills the ``.grad`` of a one-hop ``TarMACActor``.  ``critic_loss_backward`` is the centralised critic's value, advantage, value
loss and gradient in two launches (csrc/mdr_tarmac_critic_grad.hip, include/mdr_policy.h: mdr_tarmac_critic_grad), ``critic_value`` its
forward alone; the learner takes them with ``critic_backend="hip"``.  torch keeps the gradient clipping and the optimisers (or
``optimizer=FusedAdam``).  ``TarMACPPOLearner`` is the loop.  Nothing on the call path synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _learner as L
from . import _native as nat
from . import graph_update
from .tarmac import FUSED_MAX_HIDDEN, FUSED_MAX_KEY, FUSED_MAX_OBS, FUSED_MAX_VALUE, MAX_COMM, MODES, TarMACActor

# backend="auto": the kernels from this many env-steps per minibatch on (profiles/tarmac_ppo_README.md: they measured faster than
# forward(differentiable=True) + backward() at every size tried, the reference's 256 x 20 included)
AUTO_MIN_ENV_STEPS = 1
# the critic kernels' limits (include/mdr_policy.h: mdr_tarmac_critic_*)
CRITIC_MAX_JOINT, CRITIC_MAX_HIDDEN, CRITIC_MAX_AGENTS = 4096, 256, 64
# critic_backend="auto": the critic kernels for minibatches of this many env-steps (profiles/tarmac_critic_README.md: the critic's
# step measured 2.4x faster than autograd at 64 and 256 env-steps of 20 agents and 2.3x at 256 of 50 agents; at 4096 its lead of
# 1.05x is inside the comparator's spread; nothing between was measured, so auto stays with the largest size they clearly won)
CRITIC_AUTO_MIN_ENV_STEPS = 1
CRITIC_AUTO_MAX_ENV_STEPS = 256


def _head(actor):
    return actor.comm_hidden2action if actor.with_comm else actor.hidden2action


def _shape_refusal(actor, nb_houses: Optional[int] = None) -> Optional[str]:
    """Why the kernels do not take an actor of this class, these sizes, hops and comm mode, wherever its parameters are."""
    if not isinstance(actor, TarMACActor):
        return "the kernels cover a TarMACActor"
    if actor.num_hops != 1:
        return "num_hops = %d: the kernels cover one hop (forward(differentiable=True) covers more)" % actor.num_hops
    if actor.num_action != 2:
        return "the kernels cover two actions"
    F_, H = actor.num_obs, actor.hidden
    if not 1 <= F_ <= FUSED_MAX_OBS:
        return "num_obs = %d: the kernels cover at most %d features" % (F_, FUSED_MAX_OBS)
    if H < 4 or H % 4 or H > FUSED_MAX_HIDDEN:
        return "hidden_state_size = %d: the kernels cover a multiple of 4 <= %d" % (H, FUSED_MAX_HIDDEN)
    if actor.with_comm:
        K, V = actor.num_key, actor.num_value
        if K < 4 or K % 4 or K > FUSED_MAX_KEY or V < 4 or V % 4 or V > FUSED_MAX_VALUE:
            return "num_key = %d, num_value = %d: the kernels cover multiples of 4 <= %d and <= %d" % (K, V, FUSED_MAX_KEY, FUSED_MAX_VALUE)
        if actor.comm_mode not in MODES:
            return "the kernels cover the comm modes 'neighbours' and 'none'"
        if nb_houses is not None and actor.comm_mode == "neighbours" and min(actor.number_agents_comm, nb_houses - 1) > MAX_COMM:
            return "band attention covers at most %d senders per receiver" % MAX_COMM
    return None


def _refusal(actor, nb_houses: Optional[int] = None) -> Optional[str]:
    """Why the kernels do not take ``actor`` (None: they do)."""
    why = _shape_refusal(actor, nb_houses)
    if why:
        return why
    for p in _params(actor):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            return "parameters must be contiguous float32 tensors on the GPU"
    return None


def supported(actor) -> bool:
    """Do the gradient kernels take this actor?  A one-hop ``TarMACActor`` inside ``FusedTarMACActor``'s limits (num_obs <= 64,
    hidden_state_size a multiple of 4 <= 64, num_key a multiple of 4 <= 16, num_value a multiple of 4 <= 32, the modes 'neighbours'
    and 'none', with or without communication), float32 on the GPU."""
    return _refusal(actor) is None


def _params(actor) -> List[torch.Tensor]:
    """The parameters a one-hop evaluation reaches, in the order of ``actor.parameters()`` - the order of the flat gradient
    (``comm.msg_state2state`` follows them and is not reached)."""
    mods = [actor.obs2hidden, _head(actor)]
    if actor.with_comm:
        mods += [actor.comm.hidden2key, actor.comm.hidden2value, actor.comm.hidden2query]
    return [p for m in mods for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)]


def _desc(actor) -> nat.MdrTarmacNet:
    ptr = [C.c_void_p(p.data_ptr()) for p in _params(actor)]
    ptr += [None] * (20 - len(ptr))
    K, V = (actor.num_key, actor.num_value) if actor.with_comm else (4, 4)
    return nat.MdrTarmacNet(C.sizeof(nat.MdrTarmacNet), actor.num_obs, actor.hidden, K, V, actor.number_agents_comm, MODES[actor.comm_mode],
                            actor.num_hops, int(actor.with_comm), actor.comm_defect_prob, *ptr)


def actor_loss_backward(actor, state: torch.Tensor, action: torch.Tensor, old_prob: torch.Tensor, advantage: torch.Tensor,
                        clip_param: float = 0.2, index: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0,
                        want_ratio: bool = False, max_workgroups: int = 0):
    """The clipped surrogate of agents/tarmac_ppo.py:168-182 and ``backward()``: fills ``p.grad`` of every parameter of ``actor`` a
    one-hop evaluation reaches (allocated where None, overwritten otherwise; ``comm.msg_state2state`` keeps whatever ``.grad`` it had)
    and returns the loss (0-dim device tensor) [and the ratios, float32 [B, N]].  ``state`` float32 [M, N, F] (contiguous env-steps,
    any row stride >= F), ``action`` int64 [M, N], ``old_prob`` float32 [M, N]: the stored env-steps, read in place through ``index``
    (int64 [B] on the device; None: every env-step in order, B = M); ``advantage`` float32 [B, N] in minibatch order.  With
    ``comm_defect_prob > 0`` the dead senders are those of ``actor(state[index], seed=seed, step=step, differentiable=True)``."""
    what = "tarmac_ppo.actor_loss_backward"
    if not isinstance(state, torch.Tensor) or state.dim() != 3:
        raise ValueError("%s: state must be [M, N, F]" % what)
    M, N, F_len = (int(x) for x in state.shape)
    if N < 1:
        raise ValueError("%s: at least one agent per env-step" % what)
    why = _refusal(actor, N)
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev = actor.obs2hidden[0].weight.device
    if F_len != actor.num_obs or state.dtype != torch.float32 or state.device != dev:
        raise ValueError("%s: state must be a float32 [M, N, %d] tensor on %s" % (what, actor.num_obs, dev))
    ld = int(state.stride(1)) if N > 1 else (int(state.stride(0)) if M > 1 else F_len)
    if (F_len > 1 and state.stride(2) != 1) or ld < F_len or (M > 1 and N > 1 and state.stride(0) != N * ld):
        raise ValueError("%s: state rows need unit inner stride and one row stride >= F over all agents" % what)
    L.check_index(index, dev, what)
    B = int(index.shape[0]) if index is not None else M
    L.whole(action, torch.int64, M * N, dev, what, "action")
    L.whole(old_prob, torch.float32, M * N, dev, what, "old_prob")
    L.whole(advantage, torch.float32, B * N, dev, what, "advantage")
    if not 0.0 <= float(clip_param) < 1.0:
        raise ValueError("%s: clip_param must lie in [0, 1)" % what)
    desc = _desc(actor)
    floats, nbytes = _actor_sizes(desc, B, N, max_workgroups, what)
    flat = L.flat_grad(actor, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ratio = torch.empty((B, N), dtype=torch.float32, device=dev) if want_ratio else None
    with torch.cuda.device(dev):
        _actor_launch(desc, state, ld, action, old_prob, index, B, N, advantage, L.workspace(dev, nbytes), flat, loss, ratio, L.stream(dev),
                      clip_param, seed=seed, step=step, max_workgroups=max_workgroups)
    params = _params(actor)
    _zero_key_bias(actor, flat, params)
    L.publish(params, flat, L.KEEP)
    return (loss, ratio) if want_ratio else loss


def _actor_sizes(desc, B: int, N: int, max_workgroups: int = 0, what: str = "tarmac_ppo") -> Tuple[int, int]:
    """(floats of the flat gradient, bytes of workspace) of an ``mdr_tarmac_ppo_actor_grad`` call over ``B`` env-steps of ``N`` agents."""
    lib = nat.load()
    return (int(lib.mdr_tarmac_net_grad_floats(C.byref(desc))),
            L.sized(lib.mdr_tarmac_ppo_workspace_bytes(C.byref(desc), B, N, max_workgroups), what, "mdr_tarmac_ppo_workspace_bytes"))


def _actor_launch(desc, state, ld, action, old_prob, index, B, N, advantage, workspace, flat, loss, ratio, stream, clip_param, seed: int = 0,
                  step: int = 0, key: Optional[torch.Tensor] = None, step_dev: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> None:
    """mdr_tarmac_ppo_actor_grad on checked tensors and caller-owned buffers, under the device of ``state``: the eager call and the
    captured one.  ``key`` (device int32 [2] = seed lo, hi): mdr_tarmac_ppo_actor_grad_keyed, which reads the defects' key there and
    adds ``step_dev`` (one device int32, optional) to the low word of ``step`` when the kernels run."""
    lib = nat.load()
    step = C.c_uint64(int(step) & (2 ** 64 - 1))
    if key is not None:
        rc = lib.mdr_tarmac_ppo_actor_grad_keyed(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, N, L.ptr(action), L.ptr(old_prob), L.ptr(advantage),
                                                 C.c_float(clip_param), L.ptr(key), step, L.ptr(step_dev), max_workgroups, L.ptr(workspace),
                                                 L.ptr(flat), L.ptr(loss), L.ptr(ratio), stream)
        nat.check(lib, None, rc, "mdr_tarmac_ppo_actor_grad_keyed")
        return
    if step_dev is not None:
        raise ValueError("tarmac_ppo: step_dev goes with key (mdr_tarmac_ppo_actor_grad_keyed)")
    rc = lib.mdr_tarmac_ppo_actor_grad(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, N, L.ptr(action), L.ptr(old_prob), L.ptr(advantage),
                                       C.c_float(clip_param), C.c_uint64(int(seed) & (2 ** 64 - 1)), step, max_workgroups, L.ptr(workspace),
                                       L.ptr(flat), L.ptr(loss), L.ptr(ratio), stream)
    nat.check(lib, None, rc, "mdr_tarmac_ppo_actor_grad")


def _zero_key_bias(actor, flat: torch.Tensor, params: Optional[List[torch.Tensor]] = None) -> None:
    """hidden2key's last bias adds q_i . b to every score of receiver i: the softmax over its senders does not see it, and the
    reference's autograd returns exact zeros for it.  The kernels' sums leave 1e-9 of rounding there, which Adam - dividing by
    |g| + 1e-8 - turns into a tenth of a learning rate per step on a parameter the reference never moves
    (profiles/learner_golden_README.md).  The identically vanishing gradient is written as what it is: one ``zero_()`` on its slice of
    the flat gradient (nothing without communication).  ``params``: ``_params(actor)`` where the caller has it."""
    if not actor.with_comm:
        return
    params = _params(actor) if params is None else params
    at = [id(p) for p in params].index(id(actor.comm.hidden2key[2].bias))
    off = sum(p.numel() for p in params[:at])
    flat[off:off + params[at].numel()].zero_()


def _critic_layers(critic) -> Optional[List[nn.Linear]]:
    seq = getattr(critic, "critic", None)
    if not isinstance(seq, nn.Sequential) or len(seq) != 5:
        return None
    lin = [seq[0], seq[2], seq[4]]
    if not all(isinstance(m, nn.Linear) and m.bias is not None for m in lin) or not all(isinstance(seq[i], nn.ReLU) for i in (1, 3)):
        return None
    return lin


def _critic_refusal(critic) -> Optional[str]:
    """Why the critic kernels do not take ``critic`` (None: they do)."""
    lin = _critic_layers(critic)
    if lin is None:
        return "the kernels cover a TarMACCritic: `critic` = Sequential(Linear, ReLU, Linear, ReLU, Linear) with biases"
    if lin[1].in_features != lin[0].out_features or lin[2].in_features != lin[1].out_features:
        return "the three layers do not chain"
    J, N = lin[0].in_features, lin[2].out_features
    if not 1 <= N <= CRITIC_MAX_AGENTS:
        return "%d agents: the kernels cover 1 to %d" % (N, CRITIC_MAX_AGENTS)
    if J % N:
        return "the critic must read num_agents * num_obs inputs: %d is no multiple of %d" % (J, N)
    if J > CRITIC_MAX_JOINT:
        return "joint input = %d: the kernels cover at most %d columns" % (J, CRITIC_MAX_JOINT)
    if lin[0].out_features > CRITIC_MAX_HIDDEN or lin[1].out_features > CRITIC_MAX_HIDDEN:
        return "hidden layers of %d and %d units: the kernels cover at most %d" % (lin[0].out_features, lin[1].out_features, CRITIC_MAX_HIDDEN)
    if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in L.mlp_params(lin)):
        return "parameters must be contiguous float32 tensors on the GPU"
    return None


def critic_supported(critic) -> bool:
    """Do the critic kernels take this critic?  A ``TarMACCritic`` on N F <= 4096 inputs with hidden layers of at most 256 units (any
    size) and 1 <= N <= 64 agents, float32 on the GPU."""
    return _critic_refusal(critic) is None


def _critic_steps(critic, state, index, what):
    """``state`` float32 [M, N, F] with contiguous env-steps (any env-step stride >= N F) -> (dev, M, N, ld, B)."""
    why = _critic_refusal(critic)
    if why:
        raise ValueError("%s: %s" % (what, why))
    lin = _critic_layers(critic)
    dev, J, N = lin[0].weight.device, lin[0].in_features, lin[2].out_features
    F_len = J // N
    if not isinstance(state, torch.Tensor) or state.dim() != 3 or state.shape[1:] != (N, F_len) or state.dtype != torch.float32 or state.device != dev:
        raise ValueError("%s: state must be a float32 [M, %d, %d] tensor on %s" % (what, N, F_len, dev))
    M = int(state.shape[0])
    if (F_len > 1 and state.stride(2) != 1) or (N > 1 and state.stride(1) != F_len) or (M > 1 and state.stride(0) < J):
        raise ValueError("%s: state needs contiguous env-steps and an env-step stride >= N F" % what)
    L.check_index(index, dev, what)
    ld = int(state.stride(0)) if M > 1 else J
    return dev, M, N, ld, (int(index.shape[0]) if index is not None else M)


def critic_value(critic, state: torch.Tensor, index: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> torch.Tensor:
    """``critic(state[index])`` (agents/tarmac_ppo.py:97-104) from the kernels -> float32 [B, N], bit for bit the value
    ``critic_loss_backward(..., want_value=True)`` returns.  Nothing is differentiated."""
    what = "tarmac_ppo.critic_value"
    dev, M, N, ld, B = _critic_steps(critic, state, index, what)
    lib = nat.load()
    desc = L.mlp_desc(_critic_layers(critic))
    value = torch.empty((B, N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.mdr_tarmac_critic_value(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, max_workgroups, L.ptr(value), L.stream(dev))
    nat.check(lib, None, rc, "mdr_tarmac_critic_value")
    return value


def critic_loss_backward(critic, state: torch.Tensor, target: torch.Tensor, index: Optional[torch.Tensor] = None, want_value: bool = False,
                         max_workgroups: int = 0):
    """``torch.pow(target[index] - critic(state[index]), 2).mean(0).mean(0)`` and ``backward()`` of agents/tarmac_ppo.py:159-166,
    196-204: fills ``p.grad`` of the six parameters of ``critic`` (allocated where None, overwritten otherwise: views of one flat
    buffer kept with the module) and returns (loss - 0-dim device tensor -, advantage float32 [B, N] = target[index] - value, detached
    [, value float32 [B, N]]).  ``state`` float32 [M, N, F] and ``target`` float32 [M, N] are the stored env-steps and returns, read in
    place through ``index`` (int64 [B] on the device; None: every env-step in order, B = M)."""
    what = "tarmac_ppo.critic_loss_backward"
    dev, M, N, ld, B = _critic_steps(critic, state, index, what)
    L.whole(target, torch.float32, M * N, dev, what, "target")
    lin = _critic_layers(critic)
    desc = L.mlp_desc(lin)
    floats, nbytes = _critic_sizes(desc, B, max_workgroups, what)
    flat = L.flat_grad(critic, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    advantage = torch.empty((B, N), dtype=torch.float32, device=dev)
    value = torch.empty((B, N), dtype=torch.float32, device=dev) if want_value else None
    with torch.cuda.device(dev):
        _critic_launch(desc, state, ld, target, index, B, L.workspace(dev, nbytes), flat, loss, value, advantage, L.stream(dev), max_workgroups)
    L.publish(L.mlp_params(lin), flat, L.KEEP)
    return (loss, advantage, value) if want_value else (loss, advantage)


def _critic_sizes(desc, B: int, max_workgroups: int = 0, what: str = "tarmac_ppo") -> Tuple[int, int]:
    """(floats of the flat gradient, bytes of workspace) of an ``mdr_tarmac_critic_grad`` call over ``B`` env-steps."""
    lib = nat.load()
    return (int(lib.mdr_tarmac_critic_grad_floats(C.byref(desc))),
            L.sized(lib.mdr_tarmac_critic_workspace_bytes(C.byref(desc), B, max_workgroups), what, "mdr_tarmac_critic_workspace_bytes"))


def _critic_launch(desc, state, ld, target, index, B, workspace, flat, loss, value, advantage, stream, max_workgroups: int = 0) -> None:
    """mdr_tarmac_critic_grad on checked tensors and caller-owned buffers: the eager call and the captured one."""
    lib = nat.load()
    rc = lib.mdr_tarmac_critic_grad(C.byref(desc), L.ptr(state), ld, L.ptr(target), L.ptr(index), B, max_workgroups, L.ptr(workspace), L.ptr(flat),
                                    L.ptr(loss), L.ptr(value), L.ptr(advantage), stream)
    nat.check(lib, None, rc, "mdr_tarmac_critic_grad")


class TarMACPPOLearner:
    """``TarmacPPO.update`` (agents/tarmac_ppo.py:152-207) on the dict ``collect_tarmac_rollout`` returns.

    ``backend="hip"``: the actor's loss and gradient from the kernels (ValueError for an actor they refuse); ``"torch"``:
    ``forward(differentiable=True)`` under autograd (the dense formula on the CPU or with ``attention="dense"``) - the comparator, the
    CPU path and the fallback for two or more hops; ``"auto"``: the kernels where ``supported(actor)`` holds and the minibatch has at
    least ``AUTO_MIN_ENV_STEPS`` env-steps, torch otherwise.

    ``critic_backend`` chooses the centralised critic's step on its own: ``"torch"`` (the default) is autograd on
    ``critic(state[index])``; ``"hip"``: ``critic_loss_backward`` (ValueError for a critic the kernels refuse) - the critic's loss and
    gradient come first and give the advantage, then the actor's loss, clip and step, then the critic's clip and step, the
    reference's order; no ``zero_grad()`` on the critic, the kernels overwrite its gradient; ``"auto"``: the kernels where
    ``critic_supported(critic)`` holds and the minibatch has ``CRITIC_AUTO_MIN_ENV_STEPS`` to ``CRITIC_AUTO_MAX_ENV_STEPS`` env-steps
    (where they measured faster, profiles/tarmac_critic_README.md), torch otherwise.

    ``sampler="philox"``: the minibatch indices from csrc/mdr_minibatch.hip by (seed, epoch) instead of a ``torch.Generator`` (default
    ``"torch"``; ``"philox"`` under ``graph=True``).  ``graph=True``: every epoch of an update replayed from one captured graph per
    batch shape (graph_update.TarMACPPOUpdateGraph), the bits of the eager ``sampler="philox"`` update; it needs the kernels for the
    actor AND the critic (``critic_backend="hip"``, or ``"auto"`` with ``batch_size`` inside its window - a torch-autograd critic is
    refused), ``optimizer=FusedAdam`` and the philox sampler.  ``graph_max_minibatches`` bounds the minibatches (of env-steps) per
    epoch, hence the graph's node count."""

    def __init__(self, actor, critic, lr_actor: float, lr_critic: float, clip_param: float = 0.2, max_grad_norm: float = 0.5,
                 ppo_update_time: int = 10, batch_size: int = 256, backend: str = "auto", optimizer=torch.optim.Adam,
                 critic_backend: str = "torch", sampler: Optional[str] = None, graph: bool = False, graph_max_minibatches: int = 1024):
        L.check_backend(backend)
        L.check_backend(critic_backend, "critic_backend")
        sampler = L.check_sampler(sampler, graph)
        if backend == "hip":
            L.require(_refusal(actor), "TarMACPPOLearner")
        if critic_backend == "hip":
            L.require(_critic_refusal(critic), "TarMACPPOLearner", "critic_backend")
        self.actor, self.critic = actor, critic
        self.clip_param, self.max_grad_norm = float(clip_param), float(max_grad_norm)
        self.ppo_update_time, self.batch_size = int(ppo_update_time), int(batch_size)
        self.backend, self.critic_backend = backend, critic_backend
        self.actor_optimizer = optimizer(actor.parameters(), lr_actor)
        self.critic_optimizer = optimizer(critic.parameters(), lr_critic)
        self.training_step = 0
        self.sampler, self.graph, self.graph_max_minibatches = sampler, bool(graph), int(graph_max_minibatches)
        self.graph_captures = 0
        self._graphs: Dict[tuple, object] = {}
        if self.graph:
            rows = max(self.batch_size, 1)
            # backend and sampler first, then what the networks are (reasons that name the network), then the optimisers
            why = graph_update.refusal(backend, sampler, (), True) or _shape_refusal(actor)
            if not why and critic_backend == "auto":
                why = _critic_refusal(critic)
            if not why and not self.critic_uses_kernels(rows):
                why = ("critic_backend=%r steps the critic through torch's autograd at %d env-steps per minibatch, not a fixed chain of "
                       "launches; graph=True needs the critic kernels (critic_backend='hip', or 'auto' inside its window)" % (critic_backend, rows))
            if not why and backend == "auto":      # uses_kernels() asks supported(), which gives no reason
                why = _refusal(actor)
            if not why:
                why = graph_update.refusal(backend, sampler, (self.actor_optimizer, self.critic_optimizer), self.uses_kernels(rows))
            if why:
                raise ValueError("TarMACPPOLearner(graph=True): %s" % why)

    @classmethod
    def from_config(cls, tarmac_ppo_prop: dict, actor, critic, backend: str = "auto", optimizer=torch.optim.Adam,
                    critic_backend: str = "torch", sampler: Optional[str] = None, graph: bool = False,
                    graph_max_minibatches: int = 1024) -> "TarMACPPOLearner":
        """From the reference's ``config_dict["TarMAC_PPO_prop"]`` (agents/tarmac_ppo.py:39-45)."""
        p = tarmac_ppo_prop
        return cls(actor, critic, p["lr_actor"], p["lr_critic"], clip_param=p["clip_param"], max_grad_norm=p["max_grad_norm"],
                   ppo_update_time=p["ppo_update_time"], batch_size=p["batch_size"], backend=backend, optimizer=optimizer,
                   critic_backend=critic_backend, sampler=sampler, graph=graph, graph_max_minibatches=graph_max_minibatches)

    def uses_kernels(self, nb_env_steps: int) -> bool:
        if self.backend == "auto":
            return _refusal(self.actor) is None and nb_env_steps >= AUTO_MIN_ENV_STEPS
        return self.backend == "hip"

    def critic_uses_kernels(self, nb_env_steps: int) -> bool:
        if self.critic_backend == "auto":
            return CRITIC_AUTO_MIN_ENV_STEPS <= nb_env_steps <= CRITIC_AUTO_MAX_ENV_STEPS and _critic_refusal(self.critic) is None
        return self.critic_backend == "hip"

    def minibatches(self, nb_env_steps: int, seed: int, epoch: int) -> List[torch.Tensor]:
        """The index tensors of one epoch over the stored env-steps (``_learner.minibatches`` under this learner's sampler)."""
        return L.minibatches(next(self.actor.parameters()).device, nb_env_steps, self.batch_size, self.sampler, seed, epoch)

    def _capture(self, shape, nb_houses: Optional[int] = None):
        """Capture the graph of one epoch over a batch of ``shape`` = (T, A, F) - A = E N agents per step, N = ``nb_houses`` (default:
        the critic's number of agents) - without replaying it; parameters, moments and every counter are what they were."""
        T, A, F = (int(x) for x in shape)
        N = int(nb_houses) if nb_houses is not None else int(self.critic.critic[-1].out_features)
        g = graph_update.TarMACPPOUpdateGraph(self, T, A, N, F)
        self._graphs[(T, A, N, F, self.ppo_update_time, self.batch_size)] = g
        self.graph_captures += 1
        return g

    def step_minibatch(self, state, action, old_prob, target, index, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """One minibatch of agents/tarmac_ppo.py:159-207.  ``state`` [M, N, F], ``action``, ``old_prob``, ``target`` [M, N]: the whole
        buffers; ``index`` picks the env-steps.  The critic's value gives the advantage, the actor's loss is clipped and stepped, then
        the critic's.  The defects of ``comm_defect_prob > 0`` are keyed by ``(seed, training_step)``.  -> (actor loss, critic loss)."""
        critic_kernels = self.critic_uses_kernels(int(index.shape[0]))
        if critic_kernels:      # value, advantage, loss and the critic's gradient before anything steps; its clip and step stay last
            value_loss, advantage = critic_loss_backward(self.critic, state, target, index=index)
        else:
            delta = target[index] - self.critic(state[index])                   # [B, N]
            advantage = delta.detach()
        if self.uses_kernels(int(index.shape[0])):
            action_loss = actor_loss_backward(self.actor, state, action, old_prob, advantage.contiguous(), self.clip_param, index=index,
                                              seed=seed, step=self.training_step)
        else:
            kw = dict(seed=seed, step=self.training_step, differentiable=True) if state.is_cuda and self.actor.attention != "dense" else {}
            action_prob = self.actor(state[index], **kw).gather(2, action[index].unsqueeze(2)).squeeze(2)
            ratio = action_prob / old_prob[index]
            surr1 = ratio * advantage
            surr2 = torch.clamp(ratio, 1 - self.clip_param, 1 + self.clip_param) * advantage
            action_loss = -torch.min(surr1, surr2).mean()
            self.actor_optimizer.zero_grad()
            action_loss.backward()
            action_loss = action_loss.detach()
        L.clip_and_step(self.actor_optimizer, self.actor.parameters(), self.max_grad_norm)
        if not critic_kernels:
            value_loss = torch.pow(delta, 2).mean(0).mean(0)
            self.critic_optimizer.zero_grad()
            value_loss.backward()
        # (a FusedAdam's segment table covers autograd's own tensors and views of the flat buffer alike)
        L.clip_and_step(self.critic_optimizer, self.critic.parameters(), self.max_grad_norm)
        self.training_step += 1
        return action_loss, value_loss.detach()

    def update(self, batch: Dict[str, torch.Tensor], seed: int = 0, nb_houses: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``ppo_update_time`` epochs over ``batch`` (``state`` [T+1, E*N, F], ``action``, ``a_prob``, ``return`` [T, E*N]): the T E
        stored env-steps are ``batch["state"][:-1]`` viewed as [T E, N, F] and read in place, Gt is ``batch["return"]``.  ``nb_houses``
        (N): default the critic's number of agents.  -> (mean actor loss, mean critic loss - device tensors -, number of minibatches).
        ``graph=True``: the same launches replayed from a captured graph, the same bits as the eager ``sampler="philox"`` update."""
        if self.graph:
            done = graph_update.tarmac_ppo_update(self, batch, seed, nb_houses)
            if done is not None:      # None: an empty batch, nothing to replay
                return done
        states = batch["state"]
        N = int(nb_houses) if nb_houses is not None else int(self.critic.critic[-1].out_features)
        T = states.shape[0] - 1
        if states.shape[1] % N:
            raise ValueError("TarMACPPOLearner.update: %d agents per step are no whole number of envs of %d houses" % (states.shape[1], N))
        state = states[:T].reshape(-1, N, states.shape[-1])      # a view: the first T slabs of a contiguous buffer
        action = batch["action"].reshape(-1, N)
        old_prob = batch["a_prob"].reshape(-1, N)
        target = batch["return"].reshape(-1, N)
        return L.mean_losses(state.device, 2, self.ppo_update_time, lambda epoch: self.minibatches(state.shape[0], seed, epoch),
                             lambda index: self.step_minibatch(state, action, old_prob, target, index, seed=seed))
