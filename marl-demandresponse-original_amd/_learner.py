"""What the learners share (ppo, mappo, dqn, maddpg, tarmac_ppo, tarmac_a2c, graph_update): ctypes plumbing, argument checks, the
``mdr_mlp_t`` helpers, the flat gradient buffer and its publication, the samplers, clip + step, the target blend, the ring buffer.
This module imports no learner; every learner imports it.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _native as nat
from .optim import FusedAdam

# wide=True: the entry points of 65..128 input features, which have their narrow siblings' argument lists
WIDE = {"mdr_mlp_grad_floats": "mdr_mlp_wide_grad_floats", "mdr_mlp_grad_workspace_bytes": "mdr_mlp_wide_grad_workspace_bytes",
        "mdr_ppo_actor_grad": "mdr_ppo_actor_grad_wide", "mdr_ppo_critic_grad": "mdr_ppo_critic_grad_wide",
        "mdr_dqn_target": "mdr_dqn_target_wide", "mdr_dqn_grad": "mdr_dqn_grad_wide",
        "mdr_mappo_critic_grad_floats": "mdr_mappo_critic_wide_grad_floats",
        "mdr_mappo_critic_workspace_bytes": "mdr_mappo_critic_wide_workspace_bytes", "mdr_mappo_critic_grad": "mdr_mappo_critic_grad_wide"}


def fn(lib, name: str, wide: bool):
    """(the entry point ``name`` or, with ``wide``, its wide sibling; the name that was taken - what ``nat.check`` reports)."""
    if wide:
        name = WIDE[name]
    return getattr(lib, name), name


def ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_workspaces: Dict[torch.device, torch.Tensor] = {}


def workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """The one scratch buffer per device every eager gradient call shares (launches on one stream run in order)."""
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[dev] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    return ws


def sized(nbytes: int, what: str, name: str) -> int:
    """``nbytes`` as the size function ``name`` returned it; negative: it refused the sizes."""
    if nbytes < 0:
        raise ValueError("%s: %s refused the sizes" % (what, name))
    return int(nbytes)


def check_index(index: Optional[torch.Tensor], dev, what: str) -> None:
    if index is not None and (index.dtype != torch.int64 or index.dim() != 1 or index.device != dev or not index.is_contiguous()):
        raise ValueError("%s: index must be a contiguous int64 [B] tensor on the device" % what)


def whole(t, dtype, M, dev, what, name):
    if t.dtype != dtype or t.device != dev or t.numel() != M or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of %d elements on the device" % (what, name, str(dtype).replace("torch.", ""), M))
    return t


# -- mdr_mlp_t: three biased Linear layers, however the module holds them -------------------------------------------------------------
def three_linears(mods) -> Optional[List[nn.Linear]]:
    if mods is None or len(mods) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in mods):
        return None
    return list(mods)


def fc_layers(net) -> Optional[List[nn.Linear]]:
    """The layers of a net that holds them as ``fc`` (ActorMLP, CriticMLP, QNetworkMLP, DDPGNetworkMLP); None: it does not."""
    return three_linears(getattr(net, "fc", None))


def mlp_params(layers: Sequence[nn.Linear]) -> List[torch.Tensor]:
    """weight, bias of each layer: the order of ``mdr_mlp_t`` and of the flat gradient."""
    return [p for lin in layers for p in (lin.weight, lin.bias)]


def mlp_desc(layers: Sequence[nn.Linear]) -> nat.MdrMlp:
    return nat.MdrMlp(C.sizeof(nat.MdrMlp), layers[0].in_features, layers[0].out_features, layers[1].out_features, layers[2].out_features,
                      *[C.c_void_p(p.data_ptr()) for p in mlp_params(layers)])


def mlp_descs(nets: Sequence[Sequence[nn.Linear]]):
    """A host array of ``mdr_mlp_t``, one per net (the per-agent entry points: mdr_mlp_actors_sample, mdr_maddpg_target_agents)."""
    return (nat.MdrMlp * len(nets))(*[mlp_desc(layers) for layers in nets])


def mlp_sizes(desc, nb_rows: int, max_workgroups: int = 0, wide: bool = False) -> Tuple[int, int]:
    """(floats of the flat gradient, bytes of workspace) of an ``mdr_ppo_*`` / ``mdr_dqn_grad`` call over ``nb_rows`` rows."""
    lib = nat.load()
    return (int(fn(lib, "mdr_mlp_grad_floats", wide)[0](C.byref(desc))),
            int(fn(lib, "mdr_mlp_grad_workspace_bytes", wide)[0](C.byref(desc), nb_rows, max_workgroups)))


def mlp_refusal(net, outs: Tuple[int, ...], max_state: int, max_hidden: int, wide: bool = False) -> Optional[str]:
    """Why the ``mdr_mlp_t`` gradient kernels do not take ``net`` (None: they do): at most ``max_state`` input features, ``max_hidden``
    hidden units, one of ``outs`` outputs; ``wide``: also the LDS fit of the wide entry points."""
    fc = fc_layers(net)
    if fc is None:
        return "the kernels cover Linear-ReLU-Linear-ReLU-Linear (an `fc` ModuleList of three biased Linear layers)"
    if fc[1].in_features != fc[0].out_features or fc[2].in_features != fc[1].out_features:
        return "the three layers do not chain"
    if fc[0].in_features > max_state:
        return "num_state = %d: the kernels cover at most %d input features" % (fc[0].in_features, max_state)
    if fc[0].out_features > max_hidden or fc[1].out_features > max_hidden:
        return "hidden layers of %d and %d units: the kernels cover at most %d" % (fc[0].out_features, fc[1].out_features, max_hidden)
    if fc[2].out_features not in outs:
        return "%d outputs: the kernels cover an actor of 2 actions and a critic of 1 value" % fc[2].out_features
    if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in mlp_params(fc)):
        return "parameters must be contiguous float32 tensors on the GPU"
    if wide and nat.load().mdr_mlp_wide_grad_floats(C.byref(mlp_desc(fc))) < 0:
        return ("%d input features with hidden layers of %d and %d units do not fit the kernel's LDS layout"
                % (fc[0].in_features, fc[0].out_features, fc[1].out_features))
    return None


def check_rows(fc, state, index, what, num_state: Optional[int] = None):
    """``state`` float32 [M, F] rows (unit inner stride, any row stride >= F) on the device of the layers ``fc`` -> (dev, M, ld, B)."""
    dev = fc[0].weight.device
    width = fc[0].in_features if num_state is None else num_state      # of the state rows (the joint critic's input is wider)
    if state.dim() != 2 or state.shape[1] != width or state.dtype != torch.float32 or state.device != dev:
        raise ValueError("%s: state must be a float32 [M, %d] tensor on %s" % (what, width, dev))
    F_len, M = int(state.shape[1]), int(state.shape[0])
    if (F_len > 1 and state.stride(1) != 1) or (M > 1 and state.stride(0) < F_len):
        raise ValueError("%s: state rows need unit inner stride and a row stride >= F" % what)
    check_index(index, dev, what)
    ld = int(state.stride(0)) if M > 1 else F_len
    return dev, M, ld, (int(index.shape[0]) if index is not None else M)


# -- the flat gradient ------------------------------------------------------------------------------------------------------------
def flat_grad(module, floats: int, dev) -> torch.Tensor:
    """The flat float32 buffer the gradient kernels of ``module`` write, kept with the module as ``_mdr_flat_grad``."""
    flat = getattr(module, "_mdr_flat_grad", None)
    if flat is None or flat.numel() != int(floats) or flat.device != dev:
        flat = module._mdr_flat_grad = torch.empty(int(floats), dtype=torch.float32, device=dev)
    return flat


# How ``publish`` treats a parameter whose ``.grad`` is a tensor of its own (not yet the view of the flat buffer).  A ``.grad`` of None
# becomes the view in every mode.
KEEP = "keep"            # the gradient is copied into that tensor, which stays ``p.grad`` (PPO, MAPPO, DQN, MADDPG, TarMAC-PPO)
REPLACE = "replace"      # the gradient is copied into that tensor for whoever holds it; ``p.grad`` becomes the view (TarMAC A2C)
REBIND = "rebind"        # ``p.grad`` becomes the view, nothing is copied: a captured optimiser step reads these addresses (graphs)


def publish(params: Sequence[torch.Tensor], flat: torch.Tensor, mode: str) -> None:
    """``p.grad`` of ``params`` from consecutive views of ``flat``, by one of the modes above."""
    off = 0
    for p in params:
        view = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
        foreign = p.grad is not None and p.grad.data_ptr() != view.data_ptr()
        if foreign and mode != REBIND:
            p.grad.copy_(view)
        if p.grad is None or mode == REPLACE or (foreign and mode == REBIND):
            p.grad = view


# -- samplers ---------------------------------------------------------------------------------------------------------------------
def seeded_generator(seed: int, counter: int, device) -> torch.Generator:
    """A ``torch.Generator`` on ``device`` seeded by (seed, counter) - the epoch of a PPO update, the training step of a replay one."""
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(counter) * 7919 + 12345) & (2 ** 63 - 1))
    return gen


def minibatches(device, nb: int, batch_size: int, sampler: str, seed: int, epoch: int) -> List[torch.Tensor]:
    """The index tensors (int64 on ``device``) of one epoch over ``nb`` elements: a permutation drawn by (seed, epoch), cut into
    ``batch_size`` pieces; the last, shorter one is kept, as ``BatchSampler(SubsetRandomSampler(...), batch_size, False)`` keeps it
    (agents/ppo.py:140-142).  ``sampler="torch"``: ``randperm`` under ``seeded_generator``; ``"philox"``: the Feistel permutation of
    csrc/mdr_minibatch.hip, one launch - another permutation, cut the same way."""
    if sampler == "philox":
        from .graph_update import permutation      # (graph_update imports this module)
        perm = permutation(int(nb), seed, epoch, device)
    else:
        perm = torch.randperm(int(nb), generator=seeded_generator(seed, epoch, device), device=device)
    return list(torch.split(perm, batch_size))


def mean_losses(device, nb_losses: int, nb_epochs: int, minibatches_of, step) -> tuple:
    """The epoch loop of a PPO update: ``step(index)`` -> ``nb_losses`` 0-dim device tensors for every index tensor of
    ``minibatches_of(epoch)``, every epoch -> (the mean of each loss over all minibatches - device tensors -, their number)."""
    sums = [torch.zeros((), dtype=torch.float32, device=device) for _ in range(nb_losses)]
    count = 0
    for epoch in range(nb_epochs):
        for index in minibatches_of(epoch):
            for total, loss in zip(sums, step(index)):
                total += loss
            count += 1
    return tuple(total / max(count, 1) for total in sums) + (count,)


def check_backend(backend: str, name: str = "backend") -> None:
    if backend not in ("auto", "hip", "torch"):
        raise ValueError("%s must be 'auto', 'hip' or 'torch'" % name)


def check_sampler(sampler: Optional[str], graph: bool) -> str:
    """The sampler a learner runs: None is 'philox' under ``graph=True`` and 'torch' otherwise."""
    if sampler is None:
        sampler = "philox" if graph else "torch"
    if sampler not in ("torch", "philox"):
        raise ValueError("sampler must be 'torch' or 'philox'")
    return sampler


def require(why: Optional[str], learner: str, arg: str = "backend") -> None:
    """A constructor's ``backend='hip'``: the kernels must take the networks."""
    if why:
        raise ValueError("%s(%s='hip'): %s" % (learner, arg, why))


# -- clip, step, blend ------------------------------------------------------------------------------------------------------------
def clip(optimizer, params, max_grad_norm: float) -> None:
    """``clip_grad_norm_`` for an optimiser that does not clip in its own step."""
    if not isinstance(optimizer, FusedAdam):
        nn.utils.clip_grad_norm_(params, max_grad_norm)


def step(optimizer, max_grad_norm: float, **fused_kwargs) -> None:
    """FusedAdam: clip and step (and what ``fused_kwargs`` ask for) in one launch, ``.grad`` keeps the unclipped gradient (optim.py);
    any other optimiser: ``step()`` on the gradient ``clip`` has clipped."""
    if isinstance(optimizer, FusedAdam):
        optimizer.step(max_grad_norm=max_grad_norm, **fused_kwargs)
    else:
        optimizer.step()


def clip_and_step(optimizer, params, max_grad_norm: float, **fused_kwargs) -> None:
    """``clip_grad_norm_(params, max_grad_norm)`` then ``optimizer.step()``; a FusedAdam does both in one launch and is passed
    ``fused_kwargs``: the target blend (``target``, ``tau``), the bias corrections from device memory (``corrections``, ``slot``,
    ``base_dev``).  Another optimiser ignores them: its caller blends."""
    clip(optimizer, params, max_grad_norm)
    step(optimizer, max_grad_norm, **fused_kwargs)


@torch.no_grad()
def blend(target: Sequence[torch.Tensor], new: Sequence[torch.Tensor], tau: float) -> None:
    """target = (1 - tau) * target + tau * new over parallel lists of tensors (two fused launches)."""
    torch._foreach_mul_(target, 1.0 - tau)
    torch._foreach_add_(target, new, alpha=tau)


# -- replay ring ------------------------------------------------------------------------------------------------------------------
class RingBuffer:
    """``state`` / ``next_state`` float32 [capacity, *row, F], ``action`` int64 and ``reward`` float32 [capacity, *row] preallocated on
    ``device`` and written as a ring: the oldest entries are overwritten first.  The fill count and the ring position live on the
    host; no call synchronises.  A subclass gives ``row``, the shape check of ``push`` (``_rows``) and ``sample``."""

    def __init__(self, capacity: int, row: Tuple[int, ...], num_state: int, device):
        self.capacity, self.num_state = int(capacity), int(num_state)
        self.device = torch.device(device)
        shape = (self.capacity,) + tuple(row)
        self.state = torch.zeros(shape + (self.num_state,), dtype=torch.float32, device=self.device)
        self.next_state = torch.zeros(shape + (self.num_state,), dtype=torch.float32, device=self.device)
        self.action = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.reward = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self._len = 0
        self._pos = 0      # where the next entry goes

    def __len__(self) -> int:
        return self._len

    def push(self, state: torch.Tensor, action: torch.Tensor, reward: torch.Tensor, next_state: torch.Tensor) -> None:
        """``n`` entries at once, in row order, at the ring position with wrap-around; of a push larger than the capacity the last
        ``capacity`` entries stay, as with the reference's deque."""
        n = int(state.shape[0])
        rows = self._rows(n, state, next_state, action, reward)
        skip = max(n - self.capacity, 0)
        kept = n - skip
        first = min(kept, self.capacity - self._pos)      # entries up to the end of the ring; the rest wraps to its start
        for dst, src in zip((self.state, self.next_state, self.action, self.reward), rows):
            dst[self._pos:self._pos + first].copy_(src[skip:skip + first])
            if kept > first:
                dst[:kept - first].copy_(src[skip + first:])
        self._pos = (self._pos + kept) % self.capacity
        self._len = min(self._len + kept, self.capacity)

    def push_batch(self, batch: Dict[str, torch.Tensor]) -> None:
        """A collected dict (``state`` [T + 1, ..., F], ``action``, ``reward`` [T, ...]): ``state[t + 1]`` is ``next_state[t]``; the
        entries are stored in the order of the leading dimensions."""
        states = batch["state"]
        T = states.shape[0] - 1
        rows = (-1,) + tuple(states.shape[states.dim() - self.state.dim() + 1:])      # [n, *row, F]; action and reward: [n, *row]
        self.push(states[:T].reshape(rows), batch["action"].reshape(rows[:-1]), batch["reward"].reshape(rows[:-1]), states[1:].reshape(rows))

    def chronological(self) -> torch.Tensor:
        """The positions of the stored entries, oldest first (int64 on the device, computed from the host's counters)."""
        idx = torch.arange(self._len, dtype=torch.int64, device=self.device)
        return (idx + self._pos) % self.capacity if self._len == self.capacity else idx
