"""TarMAC-PPO actor and critic (agents/network.py:103-258; learner: agents/tarmac_ppo.py, loop: train_tarmacPPO.py).

``TarMACActor`` keeps the reference's module layout - ``obs2hidden``, ``comm.hidden2key|hidden2value|hidden2query|msg_state2state``,
``comm_hidden2action`` (``hidden2action`` without communication) - so a reference ``actor.pth`` loads with ``load_state_dict``.

Two ways to evaluate the attention of ``TarMAC_Comm.forward``:

``attention="dense"``  the reference's formula in torch on any device: the agents x agents score matrix per env, MaskedSoftmax
                       (utils.py:1353-1358) under the mask of ``make_masks``.  The comparator, the CPU path and the differentiable one.
``attention="band"``   CUDA: in mode "neighbours" the mask is a circular band of c + 1 senders per receiver, so the attention is
                       O(E N c) and runs as ONE HIP kernel per hop (``mdr_tarmac_comm``, include/mdr_policy.h) on keys / values
                       staged in LDS; the five small per-agent MLPs stay library GEMMs into buffers allocated once, the softmax
                       over the two logits and ``Categorical.sample`` are ``mdr_logits_sample``.  No gradients by default;
                       ``forward(..., differentiable=True)`` is the training path: the same MLPs as autograd ops around
                       ``band_attention``, whose backward is ``mdr_tarmac_comm_backward`` - O(E N c) as the forward.

``attention="gather"`` CUDA, opt-in: tarmac_comm_mode "all" (every agent of the env, one dense N x N softmax per env) and
                       "random_sample" (the receiver and c distinct others, as sparse as the band) on ``mdr_tarmac_gather`` /
                       ``gather_attention`` - the band path's chains with the other attention call.  The reference draws one
                       random mask per forward call with ``np.random`` and shares it among the batch; the port draws per env from
                       Philox, keyed by ``(seed, step, hop)`` and the receiver, as it already does for dead senders.  With
                       ``attention="auto"`` both modes stay refused; ``attention="dense"`` takes them with ``mask=`` (the
                       reference's own masks, replayable on any device).  ``FusedTarMACActor``, ``sample_env`` and the fused
                       update kernels (``tarmac_ppo``) refuse them: the learner trains through ``forward(differentiable=True)``.

The update step of the reference's learner (agents/tarmac_ppo.py:152-191) on a batch of ``collect_tarmac_rollout``, T steps of E envs::

    state = ro["state"][:-1].view(T * E, N, F)                         # one stored env-step per batch row
    action, old = ro["action"].view(T * E, N), ro["a_prob"].view(T * E, N)
    for index in minibatches(T * E):                                   # the caller's sampler, optimiser and loss terms
        probs = actor(state[index], seed=seed, step=update, differentiable=True)          # [B, N, 2], carries a grad_fn
        ratio = probs.gather(2, action[index].unsqueeze(2)).squeeze(2) / old[index]       # tarmac_ppo.py:168-186
        ...

With ``comm_defect_prob > 0`` the defects of an update are fresh draws keyed by ``(seed, step)``, the batch row standing for the env -
not the mask the rollout saw (the reference, too, redraws its mask at every forward call).  The backward of one forward call redraws
that call's mask from the same key.

``FusedTarMACActor.from_module(actor)`` evaluates the same actor WITHOUT library GEMMs: the per-agent MLPs run as HIP kernels on the
matrix cores in exact fp32 (``mdr_tarmac_actor_sample``, csrc/mdr_tarmac_mlp.hip) around the same attention kernel - three launches per
step for one hop, capturable in a graph, reachable through the C ABI alone.  ``precision="bf16x3"`` runs the same chain with every
matrix product on bf16 matrix instructions, both operands split into a bf16 head and tail (csrc/mdr_tarmac_mlp_bf16.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from .policy import OBSERVE_NUM_STATE, observe_feature_order

MODES = {"neighbours": 0, "none": 1}      # mdr_tarmac_mode
GATHER_MODES = {"all": 0, "random_sample": 1}      # mdr_tarmac_gather_mode: opt-in, attention="gather" (or "dense")
MAX_HOPS, MAX_KEY, MAX_VALUE, MAX_COMM = 4, 32, 64, 64


def band_offsets(nb_comm: int):
    """The sender offsets of ``make_masks`` (network.py:148-158) after the receiver itself: +1, -1, +2, -2, ..."""
    return [(i + 1) // 2 if i % 2 else -(i // 2) for i in range(1, int(nb_comm) + 1)]


def _mlp(n_in, n_hidden, n_out, act):
    return nn.Sequential(nn.Linear(n_in, n_hidden), act(), nn.Linear(n_hidden, n_out))


_WORKSPACES = {}      # (agents, device) -> uint8 tensor: the statistics mdr_tarmac_comm_backward passes between its two kernels


def _backward_workspace(nb_agents: int, num_key: int, num_value: int, dev) -> torch.Tensor:
    key = (int(nb_agents), dev)
    ws = _WORKSPACES.get(key)
    n = nat.load().mdr_tarmac_comm_backward_workspace_bytes(nb_agents, num_key, num_value)
    if n < 0:
        raise RuntimeError("mdr_tarmac_comm_backward_workspace_bytes refused the shape")
    if ws is None or ws.numel() < n:
        ws = _WORKSPACES[key] = torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
    return ws


def _ld(t: torch.Tensor) -> int:
    """The stride in floats from one agent's row of ``t`` [E, N, D] to the next."""
    E, N, D = t.shape
    return t.stride(1) if N > 1 else t.stride(0) if E > 1 else D


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` [E, N, D] as the kernels read it, in place where they can: unit inner stride, one row stride over all agents that is a
    multiple of 4 floats, 16-byte aligned rows.  Anything else is made contiguous first."""
    E, N, D = t.shape
    ld = _ld(t)
    ok = t.stride(2) == 1 and ld >= D and ld % 4 == 0 and t.data_ptr() % 16 == 0 and (E == 1 or N == 1 or t.stride(0) == N * ld)
    return t if ok else t.contiguous()


class _BandAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, key, value, nb_comm, mode, defect_prob, seed, step, step_dev, hop):
        E, N, K = query.shape
        V = value.shape[2]
        dev = query.device
        q, k, v = _rows(query.detach()), _rows(key.detach()), _rows(value.detach())
        out = torch.empty((E, N, V), dtype=torch.float32, device=dev)
        # the backward redraws the mask from the forward's key: keep the value the counter offset had
        step_dev = step_dev.clone() if step_dev is not None else None
        ctx.key = (int(nb_comm), int(mode), float(defect_prob), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(hop))
        ctx.step_dev = step_dev
        lib = nat.load()
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_comm(C.c_void_p(q.data_ptr()), _ld(q), C.c_void_p(k.data_ptr()), _ld(k), C.c_void_p(v.data_ptr()), _ld(v),
                                     E, N, K, V, ctx.key[0], ctx.key[1], C.c_float(ctx.key[2]), C.c_uint64(ctx.key[3]), C.c_uint64(ctx.key[4]),
                                     C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None, ctx.key[5],
                                     C.c_void_p(out.data_ptr()), V, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        nat.check(lib, None, rc, "mdr_tarmac_comm")
        ctx.save_for_backward(q, k, v, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out = ctx.saved_tensors
        E, N, K = q.shape
        V = v.shape[2]
        dev = q.device
        g = _rows(grad_out if grad_out.dtype == torch.float32 else grad_out.float())
        dq, dk = torch.empty((E, N, K), dtype=torch.float32, device=dev), torch.empty((E, N, K), dtype=torch.float32, device=dev)
        dv = torch.empty((E, N, V), dtype=torch.float32, device=dev)
        ws = _backward_workspace(E * N, K, V, dev)
        nb_comm, mode, prob, seed, step, hop = ctx.key
        step_dev = ctx.step_dev
        lib = nat.load()
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_comm_backward(C.c_void_p(q.data_ptr()), _ld(q), C.c_void_p(k.data_ptr()), _ld(k), C.c_void_p(v.data_ptr()), _ld(v),
                                              E, N, K, V, nb_comm, mode, C.c_float(prob), C.c_uint64(seed), C.c_uint64(step),
                                              C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None, hop,
                                              C.c_void_p(out.data_ptr()), V, C.c_void_p(g.data_ptr()), _ld(g), C.c_void_p(dq.data_ptr()), K,
                                              C.c_void_p(dk.data_ptr()), K, C.c_void_p(dv.data_ptr()), V, C.c_void_p(ws.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        nat.check(lib, None, rc, "mdr_tarmac_comm_backward")
        return dq, dk, dv, None, None, None, None, None, None, None


def band_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, nb_comm: int, mode: str = "neighbours",
                   defect_prob: float = 0.0, seed: int = 0, step: int = 0, step_dev: Optional[torch.Tensor] = None,
                   hop: int = 0) -> torch.Tensor:
    """The banded masked attention of ``TarMAC_Comm.forward`` with a gradient: float32 CUDA ``query``, ``key`` [E, N, K] and
    ``value`` [E, N, V] -> [E, N, V].  Forward ``mdr_tarmac_comm``, backward ``mdr_tarmac_comm_backward`` (include/mdr_policy.h; once
    differentiable), both O(E N c); the backward redraws the forward's dead-sender mask from ``(seed, step, step_dev, hop)``, nothing
    is stored but the operands and the result.  Views with unit inner stride and 16-byte aligned rows - the column blocks of a
    packed projection - are read in place through their row stride; anything else is made contiguous first.  The backward's
    workspace is cached per (agent count, device): run backwards of equal size on one stream at a time."""
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3:
            raise ValueError("%s must be a float32 CUDA tensor [E, N, D]" % name)
    if key.shape != query.shape or value.shape[:2] != query.shape[:2] or key.device != query.device or value.device != query.device:
        raise ValueError("query and key [E, N, K] and value [E, N, V] must agree in E, N, K and share a device")
    K, V = query.shape[2], value.shape[2]
    if K == 0 or K % 4 or K > MAX_KEY or V == 0 or V % 4 or V > MAX_VALUE or query.shape[1] == 0:
        raise ValueError("band attention: K a multiple of 4 <= %d, V a multiple of 4 <= %d, at least one agent" % (MAX_KEY, MAX_VALUE))
    if mode not in MODES:
        raise ValueError("mode must be 'neighbours' or 'none'")
    if int(nb_comm) < 0 or not 0.0 <= float(defect_prob) <= 1.0 or not 0 <= int(hop) < MAX_HOPS:
        raise ValueError("nb_comm >= 0, defect_prob in [0, 1], hop in 0..%d" % (MAX_HOPS - 1))
    if mode == "neighbours" and min(int(nb_comm), query.shape[1] - 1) > MAX_COMM:
        raise ValueError("band attention covers at most %d senders per receiver" % MAX_COMM)
    if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != query.device):
        raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
    return _BandAttention.apply(query, key, value, int(nb_comm), MODES[mode], float(defect_prob), seed, step, step_dev, int(hop))


_GATHER_WORKSPACES = {}      # (E, N, c, mode, device) -> uint8 tensor: statistics and index lists of mdr_tarmac_gather_backward


def _gather_workspace(E: int, N: int, K: int, V: int, nb_comm: int, mode: int, dev) -> torch.Tensor:
    n = nat.load().mdr_tarmac_gather_backward_workspace_bytes(E, N, K, V, nb_comm, mode)
    if n < 0:
        raise RuntimeError("mdr_tarmac_gather_backward_workspace_bytes refused the shape")
    key = (E, N, min(nb_comm, N - 1), mode, dev)
    ws = _GATHER_WORKSPACES.get(key)
    if ws is None or ws.numel() < n:
        ws = _GATHER_WORKSPACES[key] = torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
    return ws


def _gather_call(lib, q, k, v, ldq, ldk, ldv, E, N, K, V, nb_comm, mode, seed, step, step_dev, hop, out, ldo, dev):
    with torch.cuda.device(dev):
        rc = lib.mdr_tarmac_gather(C.c_void_p(q.data_ptr()), ldq, C.c_void_p(k.data_ptr()), ldk, C.c_void_p(v.data_ptr()), ldv, E, N, K, V,
                                   nb_comm, mode, C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint64(step & (2 ** 64 - 1)),
                                   C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None, hop,
                                   C.c_void_p(out.data_ptr()), ldo, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    nat.check(lib, None, rc, "mdr_tarmac_gather")


class _GatherAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, key, value, nb_comm, mode, seed, step, step_dev, hop):
        E, N, K = query.shape
        V = value.shape[2]
        dev = query.device
        q, k, v = _rows(query.detach()), _rows(key.detach()), _rows(value.detach())
        out = torch.empty((E, N, V), dtype=torch.float32, device=dev)
        # the backward redraws the sender sets from the forward's key: keep the value the counter offset had
        step_dev = step_dev.clone() if step_dev is not None else None
        ctx.key = (int(nb_comm), int(mode), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(hop))
        ctx.step_dev = step_dev
        _gather_call(nat.load(), q, k, v, _ld(q), _ld(k), _ld(v), E, N, K, V, ctx.key[0], ctx.key[1], ctx.key[2], ctx.key[3], step_dev,
                     ctx.key[4], out, V, dev)
        ctx.save_for_backward(q, k, v, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out = ctx.saved_tensors
        E, N, K = q.shape
        V = v.shape[2]
        dev = q.device
        g = _rows(grad_out if grad_out.dtype == torch.float32 else grad_out.float())
        dq, dk = torch.empty((E, N, K), dtype=torch.float32, device=dev), torch.empty((E, N, K), dtype=torch.float32, device=dev)
        dv = torch.empty((E, N, V), dtype=torch.float32, device=dev)
        nb_comm, mode, seed, step, hop = ctx.key
        ws = _gather_workspace(E, N, K, V, nb_comm, mode, dev)
        step_dev = ctx.step_dev
        lib = nat.load()
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_gather_backward(C.c_void_p(q.data_ptr()), _ld(q), C.c_void_p(k.data_ptr()), _ld(k), C.c_void_p(v.data_ptr()), _ld(v),
                                                E, N, K, V, nb_comm, mode, C.c_uint64(seed), C.c_uint64(step),
                                                C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None, hop,
                                                C.c_void_p(out.data_ptr()), V, C.c_void_p(g.data_ptr()), _ld(g), C.c_void_p(dq.data_ptr()), K,
                                                C.c_void_p(dk.data_ptr()), K, C.c_void_p(dv.data_ptr()), V, C.c_void_p(ws.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        nat.check(lib, None, rc, "mdr_tarmac_gather_backward")
        return dq, dk, dv, None, None, None, None, None, None


def gather_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, nb_comm: int, mode: str, seed: int = 0, step: int = 0,
                     step_dev: Optional[torch.Tensor] = None, hop: int = 0) -> torch.Tensor:
    """The attention of ``TarMAC_Comm.forward`` under the masks of tarmac_comm_mode "all" and "random_sample", with a gradient:
    float32 CUDA ``query``, ``key`` [E, N, K] and ``value`` [E, N, V] -> [E, N, V].  Forward ``mdr_tarmac_gather``, backward
    ``mdr_tarmac_gather_backward`` (include/mdr_policy.h; once differentiable, N <= 256).  "all": every agent of the env, ``nb_comm``
    ignored.  "random_sample": the receiver and min(nb_comm, N - 1) <= 64 distinct others, drawn PER ENV from Philox, keyed by
    ``(seed, step, step_dev, hop)`` and the receiver's index in the batch - the reference draws one mask per forward call with
    ``np.random`` and shares it among the whole batch; the port draws per env, as it does for dead senders.  The backward redraws the
    forward's sets from the same key, nothing is stored but the operands and the result.  No defects in these modes (nor in the
    reference's).  Views and the workspace cache as ``band_attention``."""
    for name, t in (("query", query), ("key", key), ("value", value)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3:
            raise ValueError("%s must be a float32 CUDA tensor [E, N, D]" % name)
    if key.shape != query.shape or value.shape[:2] != query.shape[:2] or key.device != query.device or value.device != query.device:
        raise ValueError("query and key [E, N, K] and value [E, N, V] must agree in E, N, K and share a device")
    K, V = query.shape[2], value.shape[2]
    if K == 0 or K % 4 or K > MAX_KEY or V == 0 or V % 4 or V > MAX_VALUE or query.shape[1] == 0:
        raise ValueError("gather attention: K a multiple of 4 <= %d, V a multiple of 4 <= %d, at least one agent" % (MAX_KEY, MAX_VALUE))
    if mode not in GATHER_MODES:
        raise ValueError("mode must be 'all' or 'random_sample'")
    if int(nb_comm) < 0 or not 0 <= int(hop) < MAX_HOPS:
        raise ValueError("nb_comm >= 0, hop in 0..%d" % (MAX_HOPS - 1))
    if mode == "random_sample" and min(int(nb_comm), query.shape[1] - 1) > MAX_COMM:
        raise ValueError("gather attention draws at most %d senders per receiver" % MAX_COMM)
    if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != query.device):
        raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
    return _GatherAttention.apply(query, key, value, int(nb_comm), GATHER_MODES[mode], seed, step, step_dev, int(hop))


class TarMACComm(nn.Module):
    """The parameters of TarMAC_Comm (network.py:103-136); evaluated by ``TarMACActor``."""

    def __init__(self, num_states: int, num_key: int, num_value: int):
        super().__init__()
        self.hidden2key = _mlp(num_states, num_states, num_key, nn.Tanh)
        self.hidden2value = _mlp(num_states, num_states, num_value, nn.Tanh)
        self.hidden2query = _mlp(num_states, num_states, num_key, nn.Tanh)
        self.msg_state2state = _mlp(num_states + num_value, num_states + num_value, num_states, nn.Tanh)


class TarMACActor(nn.Module):
    def __init__(self, num_obs: int, num_key: int = 8, num_value: int = 16, hidden_state_size: int = 64, num_action: int = 2,
                 number_agents_comm: int = 10, comm_mode: str = "neighbours", comm_defect_prob: float = 0.0, num_hops: int = 1,
                 with_comm: bool = True, attention: str = "auto", with_gru: bool = False):
        super().__init__()
        if with_gru:
            raise ValueError("with_gru is not implemented (nor is it in the reference: network.py:205-207)")
        if attention not in ("auto", "band", "dense", "gather"):
            raise ValueError("attention must be 'auto', 'band', 'dense' or 'gather'")
        if comm_mode not in MODES and not (comm_mode in GATHER_MODES and attention in ("gather", "dense")):
            raise ValueError("tarmac_comm_mode %r: only 'neighbours' and 'none' are covered ('all' and 'random_sample' are not banded)"
                             "%s" % (comm_mode, " - they are opt-in: attention='gather' or 'dense'" if comm_mode in GATHER_MODES else ""))
        if attention == "gather" and comm_mode not in GATHER_MODES:
            raise ValueError("attention='gather' evaluates the comm modes 'all' and 'random_sample'; %r is banded" % (comm_mode,))
        if not 1 <= int(num_hops) <= MAX_HOPS:
            raise ValueError("num_hops must be 1..%d (one Philox word per hop)" % MAX_HOPS)
        if not 0.0 <= float(comm_defect_prob) <= 1.0 or int(number_agents_comm) < 0:
            raise ValueError("comm_defect_prob in [0, 1], number_agents_comm >= 0")
        self.num_obs, self.num_key, self.num_value, self.hidden = int(num_obs), int(num_key), int(num_value), int(hidden_state_size)
        self.num_action = int(num_action)
        self.number_agents_comm, self.comm_mode, self.comm_defect_prob = int(number_agents_comm), comm_mode, float(comm_defect_prob)
        self.num_hops, self.with_comm, self.attention = int(num_hops), bool(with_comm), attention
        H = self.hidden
        self.obs2hidden = _mlp(num_obs, H, H, nn.ReLU)
        if self.with_comm:
            self.comm_hidden2action = _mlp(self.num_value + H, H, num_action, nn.ReLU)
            self.comm = TarMACComm(H, self.num_key, self.num_value)
        else:
            self.hidden2action = _mlp(H, H, num_action, nn.ReLU)
        self._buffers_for = None
        self._packed = None
        if attention in ("band", "gather"):
            self._check_band(None)

    @classmethod
    def from_config(cls, tarmac_ppo_prop: dict, num_obs: int, **kw) -> "TarMACActor":
        """From the reference's ``config_dict["TarMAC_PPO_prop"]`` (agents/tarmac_ppo.py:21-36).  A ``tarmac_comm_mode`` of "all" or
        "random_sample" is opt-in: ``from_config(prop, F, attention="gather")`` (the HIP kernels) or ``attention="dense"``."""
        p = tarmac_ppo_prop
        return cls(num_obs, num_key=p["key_size"], num_value=p["communication_size"], hidden_state_size=p["actor_hidden_state_size"],
                   number_agents_comm=p["number_agents_comm_tarmac"], comm_mode=p["tarmac_comm_mode"],
                   comm_defect_prob=p.get("tarmac_comm_defect_prob", 0.0), num_hops=p["comm_num_hops"], with_comm=p["with_comm"],
                   with_gru=p.get("with_gru", False), **kw)

    # ------------------------------------------------------------------------------------------------------------------ dense
    def band_mask(self, nb_agents: int, device=None) -> torch.Tensor:
        """``make_masks`` without defects: bool [receiver, sender]."""
        N = int(nb_agents)
        mask = torch.zeros((N, N), dtype=torch.bool, device=device)
        if self.comm_mode == "none":
            return mask      # no diagonal either: 0 / 0 -> NaN -> 0
        if self.comm_mode == "all":
            return ~mask
        if self.comm_mode == "random_sample":
            raise ValueError("comm mode 'random_sample' has no fixed mask: pass mask= (the draw of mdr_tarmac_gather: include/mdr_policy.h)")
        r = torch.arange(N, device=device)
        mask[r, r] = True
        for o in band_offsets(min(self.number_agents_comm, N - 1)):
            mask[r, (r + o) % N] = True
        return mask

    def _hop_dead(self, dead, hop):
        if dead is None:
            return None
        d = dead[hop] if (isinstance(dead, (list, tuple)) or dead.dim() == 3) else dead
        return d.bool()

    def dense_logits(self, obs: torch.Tensor, dead=None, mask=None) -> torch.Tensor:
        """The reference's forward up to the logits, ``obs`` [E, N, F] in the dtype of the parameters.  ``dead``: the silenced senders,
        bool [E, N] (every hop) or [num_hops, E, N] / a list per hop - required when ``comm_defect_prob > 0`` (the band path draws them
        from Philox; tests hand the same draws over).  ``mask``: the masks themselves, bool [receiver, sender] per hop, [num_hops, N, N]
        (one for the whole batch, what the reference's ``make_masks`` returns) or [num_hops, E, N, N] (one per env, what the kernels
        draw); they replace the mode's own mask - required in mode "random_sample", optional elsewhere (mode "all": ones)."""
        x = self.obs2hidden(obs)
        if not self.with_comm:
            return self.hidden2action(x)
        if mask is not None:
            mask = torch.as_tensor(mask, device=x.device).bool()
            if mask.dim() not in (3, 4) or mask.shape[0] != self.num_hops or tuple(mask.shape[-2:]) != (x.shape[1], x.shape[1]) or \
                    (mask.dim() == 4 and mask.shape[1] != x.shape[0]):
                raise ValueError("mask must be bool [num_hops, N, N] or [num_hops, E, N, N]")
            return self._dense_masked(x, mask)
        if self.comm_mode == "random_sample":
            raise ValueError("the dense path takes the masks of comm mode 'random_sample' explicitly: mask=")
        if dead is None and self.comm_defect_prob > 0.0 and self.comm_mode == "neighbours":
            raise ValueError("the dense path takes the dead-sender mask explicitly when comm_defect_prob > 0")
        E, N, _ = x.shape
        band = self.band_mask(N, x.device)
        eye = torch.eye(N, dtype=torch.bool, device=x.device)
        h, comm = x, None
        for hop in range(self.num_hops):
            if hop > 0:
                h = self.comm.msg_state2state(torch.cat([comm, h], dim=2))
            key, value, query = self.comm.hidden2key(h), self.comm.hidden2value(h), self.comm.hidden2query(h)
            mask = band
            d = self._hop_dead(dead, hop)
            if d is not None and self.comm_mode == "neighbours":
                mask = (band[None, :, :] & ~d[:, None, :]) | eye[None, :, :]      # a silenced sender still hears itself
            scores = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(self.num_key)
            s = scores - scores.max(dim=-1, keepdim=True)[0]                         # MaskedSoftmax, utils.py:1353-1358
            e = torch.exp(s) * mask.to(s.dtype)
            attn = e / e.sum(dim=-1, keepdim=True)
            attn = torch.where(torch.isnan(attn), torch.zeros_like(attn), attn)
            comm = torch.matmul(attn, value)
        return self.comm_hidden2action(torch.cat([x, comm], dim=2))

    def _dense_masked(self, x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """``dense_logits`` from the hidden state on under explicit masks, one per hop."""
        h, comm = x, None
        for hop in range(self.num_hops):
            if hop > 0:
                h = self.comm.msg_state2state(torch.cat([comm, h], dim=2))
            key, value, query = self.comm.hidden2key(h), self.comm.hidden2value(h), self.comm.hidden2query(h)
            scores = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(self.num_key)
            s = scores - scores.max(dim=-1, keepdim=True)[0]                         # MaskedSoftmax, utils.py:1353-1358
            e = torch.exp(s) * mask[hop].to(s.dtype)
            attn = e / e.sum(dim=-1, keepdim=True)
            attn = torch.where(torch.isnan(attn), torch.zeros_like(attn), attn)
            comm = torch.matmul(attn, value)
        return self.comm_hidden2action(torch.cat([x, comm], dim=2))

    # ------------------------------------------------------------------------------------------------------------------- band
    def _check_band(self, nb_agents: Optional[int]):
        if self.num_action != 2:
            raise ValueError("the band path samples between two actions")
        if not self.with_comm:
            return
        K, V, H = self.num_key, self.num_value, self.hidden
        if K % 4 or K > MAX_KEY or V % 4 or V > MAX_VALUE or H % 4:
            raise ValueError("band attention: num_key a multiple of 4 <= %d, num_value a multiple of 4 <= %d, hidden_state_size a "
                             "multiple of 4 (16-byte rows)" % (MAX_KEY, MAX_VALUE))
        c = self.number_agents_comm if nb_agents is None else min(self.number_agents_comm, nb_agents - 1)
        if self.comm_mode == "neighbours" and nb_agents is not None and c > MAX_COMM:
            raise ValueError("band attention covers at most %d senders per receiver" % MAX_COMM)
        if self.comm_mode == "random_sample" and nb_agents is not None and c > MAX_COMM:
            raise ValueError("gather attention draws at most %d senders per receiver" % MAX_COMM)

    def _use_band(self, obs) -> bool:
        if self.attention == "dense":
            return False
        if not obs.is_cuda:
            if self.attention in ("band", "gather"):
                raise ValueError("attention=%r needs the observations and the parameters on the GPU" % self.attention)
            return False
        return True

    def _pack(self):
        """[W1k; W1q; W1v] and blockdiag(W2k, W2q, W2v): the three projections are two GEMMs whose result is the packed
        [A][K + K + V] buffer the kernel reads in place.  Re-packed only when a parameter changed."""
        cm = self.comm
        mods = (cm.hidden2query, cm.hidden2key, cm.hidden2value)
        key = tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())
        if self._packed is None or self._packed[0] != key:
            H, K, V = self.hidden, self.num_key, self.num_value
            w1 = torch.cat([m[0].weight for m in mods], dim=0).detach().t().contiguous()       # [H, 3H]
            b1 = torch.cat([m[0].bias for m in mods], dim=0).detach().contiguous()
            w2 = torch.zeros((3 * H, K + K + V), dtype=w1.dtype, device=w1.device)
            col = 0
            for i, m in enumerate(mods):
                n = m[2].weight.shape[0]
                w2[i * H:(i + 1) * H, col:col + n] = m[2].weight.detach().t()
                col += n
            b2 = torch.cat([m[2].bias for m in mods], dim=0).detach().contiguous()
            self._packed = (key, w1, b1, w2, b2)
        return self._packed[1:]

    def _bufs(self, A: int, dev):
        if self._buffers_for != (A, dev):
            H, K, V = self.hidden, self.num_key, self.num_value
            f = dict(dtype=torch.float32, device=dev)
            b = {"t": torch.empty((A, H), **f), "logits": torch.empty((A, 2), **f)}
            if self.with_comm:
                b.update(cat=torch.empty((A, H + V), **f), t3=torch.empty((A, 3 * H), **f), qkv=torch.empty((A, K + K + V), **f))
                if self.num_hops > 1:
                    b.update(state=torch.empty((A, H), **f), tm=torch.empty((A, H + V), **f))
            else:
                b["h0"] = torch.empty((A, H), **f)
            self._b = b
            self._buffers_for = (A, dev)
        return self._b

    @staticmethod
    def _lin(lin, x, out, act=None):
        torch.addmm(lin.bias, x, lin.weight.t(), out=out)
        return act(out) if act is not None else out

    @torch.no_grad()
    def _band_logits(self, obs: torch.Tensor, seed: int, step: int, step_dev) -> torch.Tensor:
        """-> logits float32 [E * N, 2] (a reused buffer)."""
        if obs.dim() != 3 or obs.shape[2] != self.num_obs or obs.dtype != torch.float32:
            raise ValueError("obs must be float32 [E, N, %d]" % self.num_obs)
        E, N, _ = obs.shape
        self._check_band(N)
        dev = obs.device
        A = E * N
        lib = nat.load()
        b = self._bufs(A, dev)
        x = obs.reshape(A, self.num_obs)
        H, K, V = self.hidden, self.num_key, self.num_value
        if not self.with_comm:
            self._lin(self.obs2hidden[0], x, b["t"], torch.relu_)
            self._lin(self.obs2hidden[2], b["t"], b["h0"])
            self._lin(self.hidden2action[0], b["h0"], b["t"], torch.relu_)
            return self._lin(self.hidden2action[2], b["t"], b["logits"])
        cat = b["cat"]
        h0, comm = cat[:, :H], cat[:, H:]
        self._lin(self.obs2hidden[0], x, b["t"], torch.relu_)
        self._lin(self.obs2hidden[2], b["t"], h0)
        w1, b1, w2, b2 = self._pack()
        qkv = b["qkv"]
        h = h0
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for hop in range(self.num_hops):
            if hop > 0:      # msg_state2state(cat[comm, h]): the comm columns of W first
                m = self.comm.msg_state2state
                torch.addmm(m[0].bias, comm, m[0].weight[:, :V].t(), out=b["tm"])
                b["tm"].addmm_(h, m[0].weight[:, V:].t())
                torch.tanh_(b["tm"])
                h = self._lin(m[2], b["tm"], b["state"])
            torch.addmm(b1, h, w1, out=b["t3"])
            torch.tanh_(b["t3"])
            torch.addmm(b2, b["t3"], w2, out=qkv)
            q, k, v = qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]
            if self.comm_mode in GATHER_MODES:      # attention="gather": the same buffers, the other entry point
                _gather_call(lib, q, k, v, qkv.stride(0), qkv.stride(0), qkv.stride(0), E, N, K, V, self.number_agents_comm,
                             GATHER_MODES[self.comm_mode], seed, step, step_dev, hop, comm, cat.stride(0), dev)
                continue
            with torch.cuda.device(dev):
                rc = lib.mdr_tarmac_comm(C.c_void_p(q.data_ptr()), qkv.stride(0), C.c_void_p(k.data_ptr()), qkv.stride(0),
                                         C.c_void_p(v.data_ptr()), qkv.stride(0), E, N, K, V, self.number_agents_comm, MODES[self.comm_mode],
                                         C.c_float(self.comm_defect_prob), C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint64(step & (2 ** 64 - 1)),
                                         C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None, hop,
                                         C.c_void_p(comm.data_ptr()), cat.stride(0), stream)
            if rc != 0:
                raise RuntimeError("mdr_tarmac_comm failed: %s" % lib.mdr_status_string(rc).decode())
        self._lin(self.comm_hidden2action[0], cat, b["t"], torch.relu_)
        return self._lin(self.comm_hidden2action[2], b["t"], b["logits"])

    def _band_logits_grad(self, obs: torch.Tensor, seed: int, step: int, step_dev) -> torch.Tensor:
        """The band path as autograd ops: ``obs`` float32 [E, N, F] on the GPU -> logits [E, N, 2] with a grad_fn.  The MLPs are the
        modules themselves (F.linear + activation, fresh tensors), every hop's attention is ``band_attention`` with the defects of
        ``(seed, step, hop)``."""
        if obs.dim() != 3 or obs.shape[2] != self.num_obs or obs.dtype != torch.float32:
            raise ValueError("obs must be float32 [E, N, %d]" % self.num_obs)
        self._check_band(obs.shape[1])
        x = self.obs2hidden(obs)
        if not self.with_comm:
            return self.hidden2action(x)
        h, comm = x, None
        for hop in range(self.num_hops):
            if hop > 0:
                h = self.comm.msg_state2state(torch.cat([comm, h], dim=2))
            key, value, query = self.comm.hidden2key(h), self.comm.hidden2value(h), self.comm.hidden2query(h)
            if self.comm_mode in GATHER_MODES:
                comm = gather_attention(query, key, value, self.number_agents_comm, self.comm_mode, seed, step, step_dev, hop)
            else:
                comm = band_attention(query, key, value, self.number_agents_comm, self.comm_mode, self.comm_defect_prob, seed, step, step_dev, hop)
        return self.comm_hidden2action(torch.cat([x, comm], dim=2))

    def _head(self, logits, seed, step, step_dev, greedy, want_probs, action=None, a_prob=None):
        dev = logits.device
        A = logits.shape[0]
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        lib = nat.load()
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else action
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else a_prob
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        with torch.cuda.device(dev):
            rc = lib.mdr_logits_sample(C.c_void_p(logits.data_ptr()), logits.stride(0), A, C.c_uint64(seed & (2 ** 64 - 1)),
                                       C.c_uint64(step & (2 ** 64 - 1)), C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None,
                                       int(bool(greedy)), C.c_void_p(action.data_ptr()), C.c_void_p(a_prob.data_ptr()),
                                       C.c_void_p(probs.data_ptr()) if want_probs else None,
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError("mdr_logits_sample failed: %s" % lib.mdr_status_string(rc).decode())
        return action, a_prob, probs

    # ----------------------------------------------------------------------------------------------------------------- public
    def forward(self, obs: torch.Tensor, dead=None, seed: int = 0, step: int = 0, step_dev: Optional[torch.Tensor] = None,
                differentiable: bool = False, mask=None) -> torch.Tensor:
        """``obs`` [E, N, F] -> probabilities [E, N, 2] (TarMAC_Actor.forward).  Band path: float32 on the GPU, ``seed`` / ``step``
        key the defect draws; no gradients unless ``differentiable`` - then the result backpropagates into every parameter and into
        ``obs`` through ``band_attention`` (the update step: see the module docstring; with defects, fresh draws keyed by
        ``(seed, step)`` with the batch row as the env).  ``attention="gather"`` (comm modes "all" / "random_sample") is the band path
        with ``mdr_tarmac_gather`` / ``gather_attention`` in the attention's place; ``seed`` / ``step`` key the sender sets, one draw per
        env.  Dense path (also whenever ``dead`` or ``mask`` is given): differentiable either way; ``dead``, ``mask`` as in
        ``dense_logits``."""
        if obs.dim() != 3:
            raise ValueError("TarMAC attends over the agents of an env: obs must be [E, N, F]")
        if dead is None and mask is None and self._use_band(obs):
            if differentiable:
                return F.softmax(self._band_logits_grad(obs, seed, step, step_dev), dim=-1)
            logits = self._band_logits(obs, seed, step, step_dev)
            return self._head(logits, seed, step, step_dev, False, True)[2].view(obs.shape[0], obs.shape[1], 2)
        return F.softmax(self.dense_logits(obs, dead, mask), dim=-1)

    @torch.no_grad()
    def sample(self, obs: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: bool = False,
               dead=None, want_probs: bool = False, action: Optional[torch.Tensor] = None,
               a_prob: Optional[torch.Tensor] = None, mask=None) -> Tuple[torch.Tensor, ...]:
        """``TarmacPPO.select_actions`` (agents/tarmac_ppo.py:83-95) for every env at once: ``obs`` float32 [E, N, F] on the GPU ->
        (action uint8 [E * N], a_prob float32 [E * N][, probs [E * N, 2]]).  The draw is the one of ``FusedActor.sample`` for the same
        (seed, step, agent); ``step_dev`` (device int32) is added to ``step`` inside the kernels.  ``greedy``: the argmax, the first
        maximum on ties.  The dense path (``attention="dense"``, or ``dead`` / ``mask`` given) evaluates the reference's formula in torch
        and samples with the same kernel."""
        if not obs.is_cuda:
            raise ValueError("sampling runs on the GPU (mdr_logits_sample); the dense forward() is the CPU path")
        if self.num_action != 2:
            raise ValueError("sampling covers two actions")
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != obs.device):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        if dead is None and mask is None and self._use_band(obs):
            logits = self._band_logits(obs, seed, step, step_dev)
        else:
            logits = self.dense_logits(obs, dead, mask).reshape(-1, 2).float().contiguous()
        action, a_prob, probs = self._head(logits, seed, step, step_dev, greedy, want_probs, action, a_prob)
        return (action, a_prob, probs) if want_probs else (action, a_prob)


# ------------------------------------------------------------------------------------------------------------ fused actor
FUSED_MAX_OBS, FUSED_MAX_HIDDEN, FUSED_MAX_KEY, FUSED_MAX_VALUE = 64, 64, 16, 32


class MdrTarmacActor(C.Structure):
    """``mdr_tarmac_actor_t`` (include/mdr_policy.h), field for field."""
    _fields_ = [("struct_size", C.c_uint32), ("num_state", C.c_int32), ("hidden", C.c_int32), ("num_key", C.c_int32),
                ("num_value", C.c_int32), ("nb_comm", C.c_int32), ("mode", C.c_int32), ("num_hops", C.c_int32),
                ("with_comm", C.c_int32), ("defect_prob", C.c_float), ("greedy", C.c_int32), ("precision", C.c_int32),
                ("frag_encode", C.c_void_p), ("frag_proj", C.c_void_p), ("frag_msg", C.c_void_p), ("frag_head", C.c_void_p),
                ("vec", C.c_void_p)]


def _blocks(n: int) -> int:
    return (int(n) + 15) // 16


def _fragment(w, steps: int, nb_out: int, col):
    """One layer in MFMA fragment order (include/mdr_policy.h): ``w`` [out, in] -> float32 [steps * 64 * nb_out];
    ``col(s, g)`` -> (column of ``w`` for k-step s and lane group g, first column that is no longer this segment's)."""
    import numpy as np
    w = np.asarray(w, dtype=np.float32)
    out = np.zeros((steps, 64 * nb_out), dtype=np.float32)
    lane = np.arange(64)
    r, g = lane & 15, lane >> 4
    for s in range(steps):
        c, end = col(s, g)
        for j in range((nb_out + 3) // 4):
            wj = min(4, nb_out - 4 * j)
            for i in range(wj):
                row = 16 * (4 * j + i) + r
                ok = (row < w.shape[0]) & (c < min(end, w.shape[1]))
                out[s, 256 * j + lane * wj + i] = np.where(ok, w[np.minimum(row, w.shape[0] - 1), np.minimum(c, w.shape[1] - 1)], 0.0)
    return out.reshape(-1)


def _from_rows(steps: int, first: int, length: int):
    return lambda s, g: (first + g * steps + s, first + length)


def _from_regs(n_in: int):
    return lambda s, g: (16 * (s >> 2) + 4 * g + (s & 3), n_in)


PRECISIONS = {"fp32": 0, "bf16x3": 1}      # mdr_tarmac_precision


def observe_window_positions():
    """Float of a staged LDS row that holds normStateDict feature n of the default observation, for n < 51: the ten message records
    first, then the 11 own features (n < 11 -> 40 + n, else n - 11) - the inverse of ``policy.observe_feature_order()``, the order
    MDR_FEATURES_OBSERVE actors are packed in.  ``FusedTarMACActor.sample_env`` keeps its fragments in normStateDict order and reads
    feature n at this position instead."""
    import numpy as np
    return np.argsort(observe_feature_order(OBSERVE_NUM_STATE, 40))


def bf16_split(x):
    """float32 array -> (head, tail) bf16 bit patterns as uint16: head = bf16(x), tail = bf16(x - head), round to nearest even."""
    import numpy as np

    def bits(v):
        u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
        return ((u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) >> np.uint32(16)).astype(np.uint16)

    x = np.asarray(x, dtype=np.float32)
    head = bits(x)
    tail = bits(x - (head.astype(np.uint32) << np.uint32(16)).view(np.float32))
    return head, tail


def _fragment_bf16(w, steps: int, nb_out: int, col):
    """One layer as bf16 head / tail fragments (include/mdr_policy.h): ``w`` [out, in] -> uint32 [steps * nb_out * 512];
    ``col(s, g, j)`` -> (column of ``w`` for element j of lane group g in k-step s, whether that element is an input at all)."""
    import numpy as np
    w = np.asarray(w, dtype=np.float32)
    lane = np.arange(64)
    r, g, j = (lane & 15)[:, None], (lane >> 4)[:, None], np.arange(8)[None, :]
    vals = np.zeros((steps, nb_out, 64, 8), dtype=np.float32)
    for s in range(steps):
        c, live = col(s, g, j)
        live = live & (c < w.shape[1])
        for mb in range(nb_out):
            row = np.broadcast_to(16 * mb + r, (64, 8))
            ok = live & (row < w.shape[0])
            vals[s, mb] = np.where(ok, w[np.minimum(row, w.shape[0] - 1), np.clip(c, 0, w.shape[1] - 1)], 0.0)
    head, tail = bf16_split(vals)
    return np.ascontiguousarray(np.stack([head, tail], axis=2)).view(np.uint32).reshape(-1)      # [s][mb][t][lane][j]


def _bf16_rows(first: int, length: int):
    return lambda s, g, j: (first + 32 * s + 8 * g + j, 32 * s + 8 * g + j < length)


def _bf16_regs(nb_in: int):
    import numpy as np
    return lambda s, g, j: (16 * (2 * s + (j >> 2)) + 4 * g + (j & 3), np.broadcast_to(2 * s + (j >> 2) < nb_in, (g.shape[0], j.shape[1])))


def _pack_bf16_fragments(sd, F_, H, K, V, num_hops, with_comm):
    import numpy as np
    nbh, nbv, nbm = _blocks(H), _blocks(V), _blocks(H + V)

    def rows(w, n, c0, nbo):
        return _fragment_bf16(w, (n + 31) // 32, nbo, _bf16_rows(c0, n))

    def regs(w, nbi, nbo):
        return _fragment_bf16(w, (nbi + 1) // 2, nbo, _bf16_regs(nbi))

    res = {"frag_proj": None, "frag_msg": None}
    res["frag_encode"] = np.concatenate([rows(sd["obs2hidden.0.weight"], F_, 0, nbh), regs(sd["obs2hidden.2.weight"], nbh, nbh)])
    names = ("query", "key", "value")
    if with_comm:
        res["frag_proj"] = np.concatenate([regs(sd["comm.hidden2%s.0.weight" % n], nbh, nbh) for n in names] +
                                          [regs(sd["comm.hidden2%s.2.weight" % n], nbh, nbv if n == "value" else 1) for n in names])
        if num_hops > 1:
            w = sd["comm.msg_state2state.0.weight"]      # columns: comm (V) first, then h (H)
            res["frag_msg"] = np.concatenate([rows(w, V, 0, nbm), rows(w, H, V, nbm), regs(sd["comm.msg_state2state.2.weight"], nbm, nbh)])
        res["frag_head"] = rows(sd["comm_hidden2action.0.weight"], H + V, 0, nbh)
    else:
        res["frag_head"] = rows(sd["hidden2action.0.weight"], H, 0, nbh)
    return res


def _pack_fp32_fragments(sd, F_, H, K, V, num_hops, with_comm):
    import numpy as np
    nbh, nbv, nbm = _blocks(H), _blocks(V), _blocks(H + V)
    s1 = (F_ + 3) // 4
    res = {"frag_proj": None, "frag_msg": None}
    res["frag_encode"] = np.concatenate([_fragment(sd["obs2hidden.0.weight"], s1, nbh, _from_rows(s1, 0, F_)),
                                         _fragment(sd["obs2hidden.2.weight"], 4 * nbh, nbh, _from_regs(H))])
    names = ("query", "key", "value")
    if with_comm:
        first = [_fragment(sd["comm.hidden2%s.0.weight" % n], 4 * nbh, nbh, _from_regs(H)) for n in names]
        second = [_fragment(sd["comm.hidden2%s.2.weight" % n], 4 * nbh, nbv if n == "value" else 1, _from_regs(H)) for n in names]
        res["frag_proj"] = np.concatenate(first + second)
        if num_hops > 1:
            w = sd["comm.msg_state2state.0.weight"]      # columns: comm (V) first, then h (H)
            res["frag_msg"] = np.concatenate([_fragment(w, V // 4, nbm, _from_rows(V // 4, 0, V)),
                                              _fragment(w, H // 4, nbm, _from_rows(H // 4, V, H)),
                                              _fragment(sd["comm.msg_state2state.2.weight"], 4 * nbm, nbh, _from_regs(H + V))])
        head, d_in = "comm_hidden2action", H + V
    else:
        head, d_in = "hidden2action", H
    res["frag_head"] = _fragment(sd[head + ".0.weight"], d_in // 4, nbh, _from_rows(d_in // 4, 0, d_in))
    return res


def pack_tarmac_fragments(sd, num_obs: int, hidden: int, num_key: int, num_value: int, num_hops: int = 1, with_comm: bool = True,
                          precision: str = "fp32"):
    """A TarMAC actor's state_dict (numpy / torch, CPU) -> the five arrays of ``mdr_tarmac_actor_t`` as a dict ``frag_encode,
    frag_proj, frag_msg, frag_head, vec``; parts the actor does not have are None.  ``precision="fp32"``: float32 arrays;
    ``"bf16x3"``: the four ``frag_*`` as uint32 words of bf16 head / tail fragments, ``vec`` the same float32 array."""
    import numpy as np
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'fp32' or 'bf16x3'")
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float32) for k, v in sd.items()}
    F_, H, K, V = int(num_obs), int(hidden), int(num_key), int(num_value)
    nbh, nbv, nbm = _blocks(H), _blocks(V), _blocks(H + V)
    names = ("query", "key", "value")

    def padded(name, n):
        out = np.zeros(n, dtype=np.float32)
        if name is not None and name in sd:
            out[:sd[name].shape[0]] = sd[name]
        return out

    pack = _pack_bf16_fragments if precision == "bf16x3" else _pack_fp32_fragments
    res = pack(sd, F_, H, K, V, num_hops, with_comm)
    head = "comm_hidden2action" if with_comm else "hidden2action"
    w3, b3 = sd[head + ".2.weight"], sd[head + ".2.bias"]
    wd = np.zeros(16 * nbh, dtype=np.float32)
    wd[:H] = w3[0] - w3[1]
    c = "comm." if with_comm else None
    m = c if num_hops > 1 else None
    res["vec"] = np.concatenate([
        padded("obs2hidden.0.bias", 16 * nbh), padded("obs2hidden.2.bias", 16 * nbh),
        *[padded(c and c + "hidden2%s.0.bias" % n, 16 * nbh) for n in names],
        padded(c and c + "hidden2query.2.bias", 16), padded(c and c + "hidden2key.2.bias", 16), padded(c and c + "hidden2value.2.bias", 16 * nbv),
        padded(m and m + "msg_state2state.0.bias", 16 * nbm), padded(m and m + "msg_state2state.2.bias", 16 * nbh),
        padded(head + ".0.bias", 16 * nbh), wd, np.array([b3[0] - b3[1], 0.0, 0.0, 0.0], dtype=np.float32)])
    return res


class FusedTarMACActor:
    """A ``TarMACActor`` evaluated by ``mdr_tarmac_actor_sample`` (include/mdr_policy.h): the per-agent MLPs as three kinds of HIP
    kernels on the matrix cores around the banded attention kernel - 1 + hops + (hops - 1) + 1 launches per step, no library GEMM,
    no allocation after the first call, capturable in a graph.  ``precision="fp32"``: exact fp32 (csrc/mdr_tarmac_mlp.hip);
    ``"bf16x3"``: every matrix product on bf16 matrix instructions with both operands split into a bf16 head and tail
    (csrc/mdr_tarmac_mlp_bf16.hip; probabilities within 2e-3 relative + 2e-5 of an fp64 forward, the attention, the activations and
    the draw unchanged) - the same split as ``FusedActor``'s BF16X3 layout; the ``.precision`` attribute says which.  Inference only; to
    ``TarMACActor`` what ``FusedActor`` is to ``ActorMLP``.  Covers num_obs <= 64, hidden_state_size a multiple of 4 <= 64, num_key
    a multiple of 4 <= 16, num_value a multiple of 4 <= 32, two actions, the modes 'neighbours' and 'none'; anything else is a
    ValueError (the eager band path of ``TarMACActor`` remains for those).  ``sample_env(env, ...)`` is ``sample`` without the
    observation rows, bit for bit, for the default observation (``observe_supported``)."""

    def __init__(self, actor: "TarMACActor", precision: str = "fp32"):
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'fp32' or 'bf16x3'")
        self.actor = actor
        self.precision = precision
        self._check_shapes()
        self._packed_key = None
        self._tensors = None
        self._struct = None
        self._workspace_for = None
        self._workspace = None

    @classmethod
    def from_module(cls, actor: "TarMACActor", precision: str = "fp32") -> "FusedTarMACActor":
        return cls(actor, precision)

    def _shape(self):
        a = self.actor
        K, V = (a.num_key, a.num_value) if a.with_comm else (4, 4)      # no projections: the fields only have to be valid
        return a.num_obs, a.hidden, K, V

    def _check_shapes(self):
        a = self.actor
        if not isinstance(a, TarMACActor):
            raise ValueError("FusedTarMACActor.from_module takes a TarMACActor")
        F_, H, K, V = self._shape()
        if a.num_action != 2:
            raise ValueError("the fused TarMAC actor samples between two actions")
        if a.comm_mode not in MODES:
            raise ValueError("the fused TarMAC actor covers the comm modes 'neighbours' and 'none'")
        if not 1 <= a.num_hops <= MAX_HOPS:
            raise ValueError("num_hops must be 1..%d" % MAX_HOPS)
        if not 1 <= F_ <= FUSED_MAX_OBS:
            raise ValueError("the fused TarMAC actor covers num_obs <= %d (the eager band path has no such limit)" % FUSED_MAX_OBS)
        if H < 4 or H % 4 or H > FUSED_MAX_HIDDEN or K < 4 or K % 4 or K > FUSED_MAX_KEY or V < 4 or V % 4 or V > FUSED_MAX_VALUE:
            raise ValueError("the fused TarMAC actor covers hidden_state_size a multiple of 4 <= %d, num_key a multiple of 4 <= %d and "
                             "num_value a multiple of 4 <= %d" % (FUSED_MAX_HIDDEN, FUSED_MAX_KEY, FUSED_MAX_VALUE))

    def _pack(self):
        """Fragments on the parameters' device; re-packed only when a parameter changed."""
        a = self.actor
        params = list(a.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._packed_key != key:
            dev = params[0].device
            if dev.type != "cuda":
                raise ValueError("the fused TarMAC actor runs on the GPU: move the TarMACActor there first")
            F_, H, K, V = self._shape()
            import numpy as np
            host = pack_tarmac_fragments(a.state_dict(), F_, H, K, V, a.num_hops, a.with_comm, precision=self.precision)
            host = {n: (v.view(np.int32) if v is not None and v.dtype == np.uint32 else v) for n, v in host.items()}      # 4-byte words
            self._tensors = {n: (torch.from_numpy(v).to(dev) if v is not None else None) for n, v in host.items()}
            st = MdrTarmacActor()
            st.struct_size = C.sizeof(MdrTarmacActor)
            st.num_state, st.hidden, st.num_key, st.num_value = F_, H, K, V
            st.nb_comm, st.mode, st.num_hops, st.with_comm = a.number_agents_comm, MODES[a.comm_mode], a.num_hops, int(a.with_comm)
            st.defect_prob = a.comm_defect_prob
            st.precision = PRECISIONS[self.precision]
            for n, t in self._tensors.items():
                setattr(st, n, t.data_ptr() if t is not None else None)
            self._struct = st
            self._packed_key = key
            self._device = dev
        return self._struct

    def workspace(self, nb_agents: int, dev) -> torch.Tensor:
        """The device scratch of a sample of ``nb_agents`` agents, allocated once per (nb_agents, device)."""
        if self._workspace_for != (nb_agents, dev):
            n = nat.load().mdr_tarmac_actor_workspace_bytes(C.byref(self._pack()), nb_agents)
            if n < 0:
                raise RuntimeError("mdr_tarmac_actor_workspace_bytes refused the actor")
            self._workspace = torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
            self._workspace_for = (nb_agents, dev)
        return self._workspace

    @torch.no_grad()
    def sample(self, obs: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: bool = False,
               want_probs: bool = False, action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None):
        """As ``TarMACActor.sample``: ``obs`` float32 [E, N, F] on the GPU -> (action uint8 [E * N], a_prob float32 [E * N][, probs
        [E * N, 2]])."""
        a = self.actor
        if obs.dim() != 3 or obs.shape[2] != a.num_obs or obs.dtype != torch.float32 or not obs.is_cuda or not obs.is_contiguous():
            raise ValueError("obs must be a contiguous float32 [E, N, %d] tensor on the GPU" % a.num_obs)
        st = self._pack()
        dev = obs.device
        if dev != self._device:
            raise ValueError("obs and the actor's parameters must be on the same device")
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        E, N, _ = obs.shape
        A = E * N
        if a.with_comm and a.comm_mode == "neighbours" and min(a.number_agents_comm, N - 1) > MAX_COMM:
            raise ValueError("band attention covers at most %d senders per receiver" % MAX_COMM)
        for name, t, dt in (("action", action, torch.uint8), ("a_prob", a_prob, torch.float32)):
            if t is not None and (t.dtype != dt or t.device != dev or t.numel() != A or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous %s tensor of E * N elements on the device" % (name, dt))
        lib = nat.load()
        ws = self.workspace(A, dev)
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else action
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else a_prob
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        st.greedy = int(bool(greedy))
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_actor_sample(C.byref(st), C.c_void_p(obs.data_ptr()), E, N, C.c_uint64(seed & (2 ** 64 - 1)),
                                             C.c_uint64(step & (2 ** 64 - 1)), C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None,
                                             C.c_void_p(ws.data_ptr()), C.c_void_p(action.data_ptr()), C.c_void_p(a_prob.data_ptr()),
                                             C.c_void_p(probs.data_ptr()) if want_probs else None,
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError("mdr_tarmac_actor_sample failed: %s" % lib.mdr_status_string(rc).decode())
        return (action, a_prob, probs) if want_probs else (action, a_prob)

    def _observe_refusal(self, env) -> Optional[str]:
        """Why ``sample_env`` cannot serve ``env`` (None: it can) - the conditions ``mdr_env_tarmac_actor_sample`` checks, decided on
        the host before anything is launched."""
        if self.actor.num_obs != OBSERVE_NUM_STATE:
            return "the actor takes %d features, observe -> act builds the default observation of %d" % (self.actor.num_obs, OBSERVE_NUM_STATE)
        if getattr(env, "sharded", False):
            return "house-sharded envs are not covered"
        spec = env._obs_spec("rows")
        if spec.state_hour or spec.state_day or spec.state_solar_gain or spec.state_thermal or spec.state_hvac or spec.message_thermal or spec.message_hvac:
            return "an optional state or message column is on"
        if spec.nb_comm != 10 or spec.links or spec.random_links:
            return "the env's agents_comm_mode must be 'neighbours' with nb_agents_comm = 10"
        if spec.comm_defect_prob > 0.0:
            return "link defects on the env's messages are not covered"
        if env.nb_houses < 11:
            return "10 distinct neighbours need at least 11 houses"
        return None

    def observe_supported(self, env) -> bool:
        """Can ``sample_env`` serve ``env``?  The default observation of 51 features (no optional state / message column, ten circular
        neighbours, no link defects) of an unsharded env of at least 11 houses, and an actor with ``num_obs == 51``; the actor's own
        ``number_agents_comm``, ``comm_mode``, ``comm_defect_prob`` and hop count are the attention's and do not matter here."""
        return self._observe_refusal(env) is None

    @torch.no_grad()
    def sample_env(self, env, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: bool = False, want_probs: bool = False,
                   action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None, rows_out: Optional[torch.Tensor] = None):
        """Observe -> act (``mdr_env_tarmac_actor_sample``): ``sample(env.obs_vector("rows"), ...)`` without the rows - the first
        kernel of the chain builds the 51 features of its agents in LDS from the env's compact state.  Returns what ``sample`` returns,
        bit for bit.  ``rows_out`` (float32, contiguous, A * 51 elements): also receives the rows, bit for bit ``env.obs_vector("rows")``
        (the transition buffer's ``state``).  ``ValueError`` before any launch for an env or actor the kernel does not cover
        (``observe_supported``); no allocation after the first call when ``action`` and ``a_prob`` are passed."""
        why = self._observe_refusal(env)
        if why is not None:
            raise ValueError("FusedTarMACActor.sample_env: " + why)
        a = self.actor
        st = self._pack()
        dev = env.device
        if dev != self._device:
            raise ValueError("the env and the actor's parameters must be on the same device")
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        E, N = env.nb_envs, env.nb_houses
        A = E * N
        if a.with_comm and a.comm_mode == "neighbours" and min(a.number_agents_comm, N - 1) > MAX_COMM:
            raise ValueError("band attention covers at most %d senders per receiver" % MAX_COMM)
        for name, t, dt, n in (("action", action, torch.uint8, A), ("a_prob", a_prob, torch.float32, A),
                               ("rows_out", rows_out, torch.float32, A * OBSERVE_NUM_STATE)):
            if t is not None and (t.dtype != dt or t.device != dev or t.numel() != n or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous %s tensor of %d elements on the device" % (name, dt, n))
        lib = nat.load()
        ws = self.workspace(A, dev)
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else action
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else a_prob
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        st.greedy = int(bool(greedy))
        spec = env._obs_spec("rows")
        with torch.cuda.device(dev):
            rc = lib.mdr_env_tarmac_actor_sample(env._handle, C.byref(spec), C.byref(st), C.c_uint64(seed & (2 ** 64 - 1)),
                                                 C.c_uint64(step & (2 ** 64 - 1)), C.c_void_p(step_dev.data_ptr()) if step_dev is not None else None,
                                                 C.c_void_p(ws.data_ptr()), C.c_void_p(action.data_ptr()), C.c_void_p(a_prob.data_ptr()),
                                                 C.c_void_p(probs.data_ptr()) if want_probs else None,
                                                 C.c_void_p(rows_out.data_ptr()) if rows_out is not None else None,
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc == nat.MDR_ERR_UNSUPPORTED:
            raise ValueError("FusedTarMACActor.sample_env: " + lib.mdr_last_error(env._handle).decode())
        nat.check(lib, env._handle, rc, "mdr_env_tarmac_actor_sample")
        return (action, a_prob, probs) if want_probs else (action, a_prob)

    def probs(self, obs: torch.Tensor, seed: int = 0, step: int = 0, step_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``obs`` [E, N, F] -> probabilities [E, N, 2] (``seed`` / ``step`` key the defect draws)."""
        return self.sample(obs, seed, step, step_dev, want_probs=True)[2].view(obs.shape[0], obs.shape[1], 2)


class TarMACCritic(nn.Module):
    """network.py:241-258: the centralised critic, all observations of an env -> one value per agent.  Plain torch."""

    def __init__(self, num_agents: int, num_obs: int, hidden_layer_size: int = 64):
        super().__init__()
        self.critic = nn.Sequential(nn.Linear(num_obs * num_agents, hidden_layer_size), nn.ReLU(),
                                    nn.Linear(hidden_layer_size, hidden_layer_size), nn.ReLU(),
                                    nn.Linear(hidden_layer_size, num_agents))

    def forward(self, obs):
        return self.critic(obs.reshape(obs.shape[0], -1))
